"""Trees of height 4 to 8 on the GPU, from built page images
(tests/image_builder.py), against the CPU oracle.

A tree built by inserts in a test's time has root level 2 or 3, so the level
loops of the writers (propagate / apply_run in split_wave.h, run_levels and
the phase tickets in insert.hip, write_new_root, parent_of, the deletes'
descent) and of the readers (get, locate, range, scan, k_top, the leaf
directory's builds and rebuilds) never ran above level 3 in a test.  The
images here are tall and thin: one full page per level on the path to one
full leaf (the hot leaf), two entries per leaf elsewhere.  40 new keys in the
hot leaf split every level of the path; a full root grows.

The oracle wraps the same image and applies the same chunks.  One shape is
out of its reach: like the reference, whose path stack has an entry per level
0..6, it cannot hand a separator to a level-7 page (it asserts).  For the
level-7 writer case the expected contents therefore come from an oracle
holding the same pairs in a tree of its own making, and the expected shape
(the half-full root absorbs: root level 7 stays) is asserted as such.

Every image passes the oracle's structural check before a GPU sees it.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model  # noqa: E402
from arena_model import hot_chunk  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import assert_same, dev, gpu_search, host, lib_ok, SENT, U64  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402
from scan_model import ScanModel  # noqa: E402
import state_model  # noqa: E402

KEY_MAX = (1 << 64) - 1
ARENA = 64 << 20
MAX_BATCH = 1 << 14
SPARE = 16 << 20
HANDOFF = 0x100  # kErrHandoff

# shm__upper_force flags of the four writer modes
MODES = {"default": 0, "upper": 4, "lists": 6, "abort": 7}


@functools.lru_cache(maxsize=None)
def tall(root_level, path, root_full, page_ver=1):
    """the image, built once per shape (read only: every user copies it)"""
    img, root, info = ib.build_tall(root_level, path, root_full, page_ver=page_ver)
    img.setflags(write=False)
    return img, root, info


def load(root_level, path, root_full, page_ver=1, wrapped=True, **tree_args):
    """The image in a Tree and in an oracle.  The oracle's structural check
    passes before the GPU sees the image.  wrapped False: the oracle holds
    the same pairs in a tree built by its own inserts (for the chunks a
    wrapped level-7 root cannot take)."""
    img, root, info = tall(root_level, path, root_full, page_ver)
    orc = OracleTree(image=img, root_ptr=root, spare_bytes=SPARE)
    rc, shape = orc.check()
    assert rc == 0, rc
    assert shape == {"leaves": info["leaves"], "internal": info["internal"],
                     "keys": info["n_keys"], "height": root_level + 1}
    if not wrapped:
        orc.close()
        orc = OracleTree(ARENA)
        orc.apply_batch(info["keys"], info["vals"])
    t = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, **tree_args)
    t.load_image(img, root)
    assert t.check() == {"leaves": info["leaves"], "internal": info["internal"],
                         "keys": info["n_keys"]}
    assert t.stats()["height"] == root_level + 1 and t.stats()["root_level"] == root_level
    return t, orc, info


def probes(info, stored):
    """every stored key and its neighbours, the ends of the key space, and
    both fences of every path page with their neighbours"""
    fences = np.array([f for lvl in info["path"] for f in info["path"][lvl][1:]], dtype=U64)
    p = np.concatenate([stored, stored + U64(1), stored - U64(1), info["deleted"],
                        np.array([0, KEY_MAX - 1], dtype=U64),
                        fences, fences + U64(1), fences - U64(1)])
    return np.unique(p[p != U64(KEY_MAX)])


def check_scans(t, model, lo, limit):
    n = lo.size
    keys = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
    vals = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
    counts = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    c, k, v = t.scan_batch(dev(lo), limit, keys=keys, vals=vals, counts=counts).result()
    c, k, v = c.cpu().numpy(), host(k), host(v)
    mc, mk, mv, w = model.scan(lo, limit)
    bad = np.nonzero(c != mc)[0]
    assert bad.size == 0, (f"limit {limit}: {bad.size} counts differ, first lo="
                           f"{int(lo[bad[0]]):#x} gpu={c[bad[0]]} model={mc[bad[0]]}")
    assert np.array_equal(k[w], mk[w]) and np.array_equal(v[w], mv[w]), f"limit {limit}"
    assert (k[~w] == U64(SENT)).all() and (v[~w] == U64(SENT)).all()


def check_reads(t, orc, info, what, scans=True):
    """Every reader against the oracle's contents as they are now."""
    ok, ov = orc.dump()
    model = ScanModel(ok, ov)
    probe = probes(info, model.keys)
    want = orc.search_batch(probe)
    assert int(want[1].sum()) == model.keys.size
    assert_same(probe, *want, *gpu_search(t, probe), what)
    # the same gets in another order (a batch the ordering pass has to sort)
    mix = np.random.default_rng(3).permutation(probe.size)
    gv, gf = gpu_search(t, probe[mix])
    assert_same(probe[mix], want[0][mix], want[1][mix], gv, gf, what + ", shuffled")
    if scans:
        # windows that start left of the hot leaf and end right of it, from
        # a few keys to the whole key space
        hot_lo, hot_hi = info["hot_lo"], info["hot_hi"]
        step = info["step"]
        lo = [max(hot_lo - w * step, 0) for w in (1, 3, 70, 1000)] + [0, hot_lo, hot_lo + 1]
        hi = [min(hot_hi + w * step, KEY_MAX - 1) for w in (1, 3, 70, 1000)] + \
            [KEY_MAX - 1, hot_hi, hot_hi - 1]
        lo, hi = np.array(lo, dtype=U64), np.array(hi, dtype=U64)
        counts, vals = t.range_query_batch(dev(lo), dev(hi))
        counts, vals = counts.cpu().numpy(), host(vals)
        a = np.searchsorted(model.keys, lo, side="left")
        b = np.searchsorted(model.keys, hi, side="right")
        assert np.array_equal(counts, b - a), (what, counts, b - a)
        # the order (leaf order, then slot order) belongs to the page image:
        # the reference scan over the GPU's own pages gives it
        own = OracleTree(image=t.dump_image()[0], root_ptr=t.stats()["root_ptr"])
        off = 0
        for i in range(lo.size):
            got = vals[off:off + counts[i]]
            assert np.array_equal(np.sort(got), np.sort(model.vals[a[i]:b[i]])), (what, i)
            ref, n = own.range_query(int(lo[i]), int(hi[i]), cap=1 << 16)
            assert n == counts[i] and np.array_equal(got, ref), (what, i)
            off += counts[i]
        own.close()
        # a few thousand starts all over the key space, and every probe
        # within three keys of the hot leaf
        near = (probe >= U64(max(hot_lo - 3 * step, 0))) & \
            (probe <= U64(min(hot_hi + 3 * step, KEY_MAX)))
        froms = np.unique(np.concatenate([probe[::probe.size // 3000 + 1], probe[near],
                                          np.array([hot_lo, hot_hi, KEY_MAX], dtype=U64)]))
        assert froms.size <= MAX_BATCH
        for limit in (1, 54, 200):
            check_scans(t, model, froms, limit)
        froms = froms[froms != U64(KEY_MAX)]
        found, k, v = t.lower_bound_batch(dev(froms))
        at = np.searchsorted(model.keys, froms, side="left")
        has = at < model.keys.size
        assert np.array_equal(found.cpu().numpy(), has), what
        at = np.minimum(at, model.keys.size - 1)
        assert np.array_equal(host(k)[has], model.keys[at][has]), what
        assert np.array_equal(host(v)[has], model.vals[at][has]), what
    if t.dir_stats()["exact"]:  # otherwise the entries are starts, trusted for nothing
        dv = t.dir_verify()
        assert dv["checked"] > 0, (what, dv)
        assert dv["bad_lists"] == dv["bad_pairs"] == dv["bad_fps"] == dv["bad_vals"] == 0, (what, dv)
        bad, _ = dir_model.check_tree(t, ok, ov)
        assert not bad, (what, bad[:4])
    assert t.last_error()["bits"] == 0, (what, t.last_error())
    return probe


def enter_read_phase(t, probe):
    for _ in range(6):
        gpu_search(t, probe[:512])
    if t.dir_stats()["form"] != "none":
        assert t.dir_stats()["exact"], t.dir_stats()


READ_TREES = {
    "default": {},
    "no_dir": {"leaf_dir": False, "sort_gets": False},
    "sorted": {"sort_gets": True},
    "unsorted": {"sort_gets": False},
    "top_lds": {"top_lds": True, "leaf_dir": False, "sort_gets": True},
}
READ_CASES = [(lvl, path, kind)
              for lvl, path in ((3, "middle"), (5, "left"), (5, "middle"), (5, "right"),
                                (7, "right"))
              for kind in ("default", "no_dir", "sorted", "unsorted")] + \
             [(5, "middle", "top_lds"), (7, "right", "top_lds")]


@pytest.mark.parametrize("root_level,path,kind", READ_CASES)
def test_readers_on_a_tall_tree(lib_ok, root_level, path, kind):
    """Gets, range scans, ordered scans and lower bounds on a loaded image of
    root level 3, 5 or 7, as loaded and again in a read phase (the default
    tree then answers from the pair-form directory and the bucket table)."""
    t, orc, info = load(root_level, path, root_level < 7, **READ_TREES[kind])
    probe = check_reads(t, orc, info, "as loaded")
    enter_read_phase(t, probe)
    if kind == "default":
        assert t.vt_stats()["trusted"], t.vt_stats()
        assert t.dir_stats()["form"] == "pairs", t.dir_stats()
    check_reads(t, orc, info, "read phase")
    assert t.check() == {"leaves": info["leaves"], "internal": info["internal"],
                         "keys": info["n_keys"]}
    assert t.stats()["height"] == root_level + 1
    orc.close()
    t.close()


def spread_chunk(info, orc):
    """60 absent keys in each of 150 thin leaves spread over the whole key
    range (30 would leave every leaf unsplit: 2 + 30 < 54), and 200 deletes
    of stored keys."""
    low = info["leaf_lo"]
    thin = np.nonzero((info["leaf_live"] == 2) & (low != U64(info["hot_lo"])))[0]
    pick = thin[np.linspace(1, thin.size - 2, 150).astype(np.int64)]
    assert np.unique(pick).size == 150
    # a thin leaf's keys are its lowest fence and that + step
    sub = info["step"] // 64
    new = (low[pick][:, None] + U64(sub) * np.arange(1, 61, dtype=U64)[None, :]).ravel()
    stored, _ = orc.dump()
    assert not np.isin(new, stored).any()
    dele = np.sort(stored)[np.linspace(0, stored.size - 1, 200).astype(np.int64)]
    keys = np.concatenate([new, dele])
    vals = np.concatenate([new ^ U64(0x6666), np.zeros(dele.size, dtype=U64)])
    o = np.random.default_rng(11).permutation(keys.size)
    return keys[o], vals[o]


def assert_side(t, what, pages=None):
    """The side state of the pages against the pages themselves
    (tests/state_model.py): every leaf summary line and occupancy bound of
    the first `pages` arena pages (None: the pages in use) is sound for the
    dumped image; the structural check passes and no error bit is set.
    Returns (image, root, lines, hw)."""
    img, root = t.dump_image()
    lines, hw, si = t.side_dump(pages)
    assert si["next_page"] * ib.PAGE == img.size, (what, si, img.size)
    bad = state_model.side_violations(img, root, lines, hw, si["next_page"])
    assert bad == [], (what, len(bad), bad[:12])
    t.check()
    assert t.last_error()["bits"] == 0, (what, t.last_error())
    return img, root, lines, hw


def check_contents(t, orc, what):
    """The contents three ways: the numpy reader of the GPU's pages, the
    oracle's own reader of them, and the GPU's gets of the oracle's keys;
    and the side state of the pages."""
    ok, ov = orc.dump()
    img, root, _, _ = assert_side(t, what)
    dir_model.Image(img, root).assert_equals(ok, ov)
    again = OracleTree(image=img, root_ptr=root)
    rc, shape = again.check()
    assert rc == 0, (what, rc)
    ak, av = again.dump()
    o, w = np.argsort(ak), np.argsort(ok)
    assert np.array_equal(ak[o], ok[w]) and np.array_equal(av[o], ov[w]), what
    again.close()
    gv, gf = gpu_search(t, ok)
    assert gf.all() and np.array_equal(gv, ov), what
    st = t.check()
    assert st["keys"] == ok.size, (what, st, ok.size)
    return shape


def apply_hot_chunk(t, orc, info, mode, grows, wrapped=True):
    """The hot chunk on both trees in one of the four writer modes; the
    device error, the shape and the contents after it."""
    H = shm._hooks()
    root_level = info["root_level"]
    pages = t.stats()["pages_used"]
    keys, vals = hot_chunk(info)
    assert H.shm__upper_force(t.h, MODES[mode]) == 0
    t.insert_batch(dev(keys), dev(vals))
    orc.apply_batch(keys, vals)
    e = t.last_error(reset=True)
    if mode == "abort":
        assert e["bits"] == HANDOFF and e["resumed"] == 1 and e["status"] == shm.SHM_OK, e
        assert e["chunk"] == t.last_chunk(), e
    else:
        assert e["bits"] == 0 and e["resumed"] == 0, e
    st = t.stats()
    want_level = root_level + (1 if grows else 0)
    if wrapped:
        rc, oshape = orc.check()
        assert rc == 0 and orc.root_level == want_level and oshape["height"] == want_level + 1
    assert st["root_level"] == want_level and st["height"] == want_level + 1, st
    # a page per level that split (0 .. root_level, the root only if it grew)
    # and the new root
    assert st["pages_used"] >= pages + root_level + (2 if grows else 0), (st, pages)
    shape = check_contents(t, orc, f"hot chunk, {mode}")
    assert shape["height"] == want_level + 1
    return keys


WRITE_CASES = [(3, "left", True), (3, "middle", True), (3, "right", True),
               (6, "middle", True), (7, "middle", False)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("root_level,path,root_full", WRITE_CASES)
def test_splits_up_a_tall_tree(lib_ok, root_level, path, root_full, mode):
    """40 new keys in the hot leaf (with deletes, overwrites and duplicates
    elsewhere) split the path page of every level: a full root of level 3 or
    6 grows to 4 or 7, a half-full root of level 7 absorbs the separator of
    its level-6 child.  Then every reader on the directory as the chunk left
    it and in a read phase, and a second chunk that splits 150 thin leaves
    all over the key range."""
    wrapped = root_level < 7
    t, orc, info = load(root_level, path, root_full, wrapped=wrapped)
    # a directory for the chunk to keep, and for its rebuild from the hint
    gpu_search(t, info["keys"][:256])
    apply_hot_chunk(t, orc, info, mode, grows=root_full, wrapped=wrapped)
    # the chunk kept the directory it found: still exact, and checked as such
    assert t.dir_stats()["exact"], t.dir_stats()
    probe = check_reads(t, orc, info, "after the hot chunk")
    enter_read_phase(t, probe)
    check_reads(t, orc, info, "after the hot chunk, read phase")

    pages = t.stats()["pages_used"]
    level = t.stats()["root_level"]
    keys, vals = spread_chunk(info, orc)
    t.insert_batch(dev(keys), dev(vals))
    orc.apply_batch(keys, vals)
    assert t.last_error()["bits"] == 0, t.last_error()
    st = t.stats()
    assert st["root_level"] == level and st["pages_used"] >= pages + 150, (st, pages)
    if wrapped:
        assert orc.root_level == level
    check_contents(t, orc, "spread chunk")
    probe = check_reads(t, orc, info, "after the spread chunk")
    enter_read_phase(t, probe)
    check_reads(t, orc, info, "after the spread chunk, read phase")
    orc.close()
    t.close()


def test_queued_reads_see_the_grown_tree(lib_ok):
    """The growing chunk, a search and a scan queued with no host wait in
    between, then one synchronize: both reads see the tree of root level 7."""
    t, orc, info = load(6, "middle", True)
    keys, vals = hot_chunk(info)
    orc.apply_batch(keys, vals)
    ok, ov = orc.dump()
    model = ScanModel(ok, ov)
    probe = probes(info, model.keys)
    froms = np.concatenate([probe[::7], np.array([info["hot_lo"]], dtype=U64)])
    assert froms.size <= MAX_BATCH
    limit = 54
    dk, dv, dp, df = dev(keys), dev(vals), dev(probe), dev(froms)
    gv = torch.empty_like(dp)
    gf = torch.empty(dp.numel(), dtype=torch.uint8, device="cuda")
    t.insert_batch_async(dk, dv)
    t.search_batch(dp, gv, gf)
    pend = t.scan_batch(df, limit)
    t.synchronize()
    assert t.last_error()["bits"] == 0, t.last_error()
    assert_same(probe, *orc.search_batch(probe), host(gv), gf.cpu().numpy(), "queued search")
    c, k, v = pend.result()
    mc, mk, mv, w = model.scan(froms, limit)
    assert np.array_equal(c.cpu().numpy(), mc)
    assert np.array_equal(host(k)[w], mk[w]) and np.array_equal(host(v)[w], mv[w])
    assert t.stats()["root_level"] == 7 and orc.root_level == 7
    check_contents(t, orc, "queued chunk")
    orc.close()
    t.close()


def test_page_versions_wrap(lib_ok):
    """Every page at version 255: the pages the chunk writes wrap to a small
    version with front == rear (the wrapped oracle's check reads both), and
    the readers take the rewritten pages."""
    t, orc, info = load(3, "middle", True, page_ver=255)
    gpu_search(t, info["keys"][:256])  # a directory for the chunk to keep
    apply_hot_chunk(t, orc, info, "default", grows=True)
    img, root = t.dump_image()
    pg = img.reshape(-1, ib.PAGE)
    for lvl, (page, _, _) in info["path"].items():
        front = int(pg[page, ib.OFF_FRONT_VER])
        rear = int(pg[page, ib.OFF_LEAF_REAR if lvl == 0 else ib.OFF_INTERNAL_REAR])
        print(f"level {lvl} path page {page}: front {front} rear {rear}")
        assert front == rear and front < 255, (lvl, page, front, rear)
    check_reads(t, orc, info, "after the wrap")
    orc.close()
    t.close()
