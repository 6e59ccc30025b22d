"""The page arena runs out: status, tree shape and every reader afterwards.

shm_insert_batch documents SHM_ENOMEM ("the splits that did not fit are left
unapplied"), and three code paths implement it: the room test of the upsert
kernel's early splits (split_wave.h split_early), the all-or-nothing test of
k_upper's leaf level (insert.hip) and the bump allocator of the internal
levels (split_wave.h alloc_pages), after whose failure new pages hang on
their left sibling alone.  Every other GPU test gives its tree megabytes for
a few hundred pages, so none of them ran.

The truth of every case is the page image the failed chunk left, read by the
CPU oracle and by nothing else (T): its leaf-chain dump, cross-checked with
its search from the root over all probes.  What the GPU's readers answer is
compared with T, never with the GPU's own gets; what T may hold is judged by
arena_model.classify_outcome against the oracle's contents without and with
the chunk.

  A  exact arenas: the image of root level 2 (tests/image_builder.py) in an
     arena of `spare` free pages, the hot chunk in each writer mode.  `need`,
     the pages the chunk takes in that mode, comes from a control run with
     room; the spares 0 .. need are all run (need itself: success with the
     arena exactly full, the `<=` of all three allocators; above it: success
     with pages left).
  B  arenas of 3 and 63 usable pages filled by chunks of hashed keys.
  C  a chunk rejected whole for kKeyMax beside a trusted bucket table.

One departure from the plain reading of "the hot chunk again returns
SHM_ENOMEM": where the failed chunk did store its new keys (the leaf level
fitted and an internal level did not), the same chunk again finds them stored
and has nothing left to split, so it must return SHM_OK; a chunk that splits
more thin leaves than pages are left then takes its place.
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
import get_paths  # noqa: E402
import gpu_helpers  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import assert_same, dev, gpu_search, host, lib_ok, U64  # noqa: E402
import state_model as sm  # noqa: E402
import test_gpu_tall as tall  # noqa: E402
import valtab_model  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

PAGE = 1024
KEY_MAX = (1 << 64) - 1
NOMEM, HANDOFF, KEYMAX_BIT = 0x80, 0x100, 1 << 31  # kErrNoMem, kErrHandoff, kErrKeyMax
ROOM = 64 * PAGE  # free pages of the oracles that take a chunk whole
SPARES = tuple(range(8))  # the sweep; the test fails if `need` is not inside it

def contents(orc):
    k, v = orc.dump()
    o = np.argsort(k)
    return k[o], v[o]


def failed(fn, rc):
    with pytest.raises(shm.ShermanError) as e:
        fn()
    assert e.value.rc == rc, (e.value.rc, rc)


def error_state(t, rc, bit, allowed):
    """the device error block after a failed synchronising call; then reset
    (the sticky word of stats() stays)"""
    e = t.last_error()
    assert e["bits"] & bit and not e["bits"] & ~allowed, e
    assert e["status"] == rc and e["chunk"] == t.last_chunk(), (e, t.last_chunk())
    t.last_error(reset=True)
    st = t.stats()
    assert st["last_error"] & bit, st
    assert st["pages_used"] <= st["pages_capacity"], st
    return st


def truth(t, info, also):
    """T: the oracle over the dumped image (with free pages after it, for the
    ops applied to both later).  Its structural check passes, the GPU's own
    check and shape agree with it, and its dump and its search from the root
    agree over every probe, and the side state of the pages is sound for the
    image (tall.assert_side: the caller has read and reset the failed chunk's
    error bits).  Returns T, its sorted contents, the probes."""
    img, root, _, _ = tall.assert_side(t, "the dumped image")
    T = OracleTree(image=img, root_ptr=root, spare_bytes=ROOM)
    rc, shape = T.check()
    assert rc == 0, rc
    st = t.stats()
    assert st["root_level"] == T.root_level and st["height"] == shape["height"], (st, shape)
    assert t.check() == {k: shape[k] for k in ("leaves", "internal", "keys")}
    assert shape["leaves"] + shape["internal"] <= st["pages_used"] <= st["pages_capacity"]
    tk, tv = contents(T)
    probe = tall.probes(info, np.unique(np.concatenate([tk] + [np.asarray(a, dtype=U64)
                                                               for a in also])))
    v, f = T.search_batch(probe)
    assert np.array_equal(probe[f != 0], tk) and np.array_equal(v[f != 0], tv)
    return T, (tk, tv), probe


def table_clean(t, kv, want_trusted):
    bad, vinfo = valtab_model.check_tree(t, *kv)
    assert bad == [], bad[:8]
    if want_trusted:
        assert vinfo["trusted"], vinfo
        assert t.dir_stats()["exact"], t.dir_stats()


def readers(t, T, info, probe, what, monkeypatch):
    """every reader against T: on the directory and the table as the failed
    chunk left them, in a read phase, and from two trees without them"""
    want = T.search_batch(probe)
    assert_same(probe, *want, *gpu_search(t, probe), what)
    tall.check_reads(t, T, info, what)
    tall.enter_read_phase(t, probe)
    table_clean(t, contents(T), False)
    first = gpu_search(t, probe)
    assert_same(probe, *want, *first, what + ", read phase")
    tall.check_reads(t, T, info, what + ", read phase")
    img, root = t.dump_image()
    monkeypatch.setenv("SHM_VALTAB", "0")
    no_table = shm.Tree(arena_bytes=img.nbytes + 4 * PAGE, max_batch=tall.MAX_BATCH)
    monkeypatch.delenv("SHM_VALTAB")
    no_dir = shm.Tree(arena_bytes=img.nbytes + 4 * PAGE, max_batch=tall.MAX_BATCH, leaf_dir=False)
    for other, name in ((no_table, "no table"), (no_dir, "no directory")):
        other.load_image(img, root)
        for _ in range(7):  # as loaded, and in its read phase
            got = gpu_search(other, probe)
        assert not other.vt_stats()["trusted"], name
        assert_same(probe, *first, *got, f"{what}, {name} against the first tree")
        other.close()


def key_with_room(t, candidates):
    """the first candidate a copy of the tree's image takes without a new page"""
    img, root = t.dump_image()
    for k in candidates:
        o = OracleTree(image=img, root_ptr=root, spare_bytes=ROOM)
        n0 = o.image().nbytes
        assert not o.search(int(k))[0]
        o.insert(int(k), 1)
        grew = o.image().nbytes != n0
        o.close()
        if not grew:
            return np.array([k], dtype=U64)
    raise AssertionError("no candidate key fits its leaf")


def handle_afterwards(t, T, kv, info, chunk, not_stored, same_again, more, candidates, force,
                      judge):
    """The handle after the failure: the failed chunk again (in the same
    writer mode), then overwrites, deletes and one new key where there is
    room, on the GPU and on T."""
    keys, vals = chunk
    st = t.stats()
    free = st["pages_capacity"] - st["pages_used"]
    assert shm._hooks().shm__upper_force(t.h, force) == 0
    if not_stored and (same_again or free == 0):
        failed(lambda: t.insert_batch(dev(keys), dev(vals)), shm.SHM_ENOMEM)
        error_state(t, shm.SHM_ENOMEM, NOMEM, NOMEM | HANDOFF)
        assert t.stats()["pages_used"] == st["pages_used"]
        tall.check_contents(t, T, "the failed chunk again")
    else:
        # nothing left to split (or pages left for some of it): never SHM_EIO
        try:
            t.insert_batch(dev(keys), dev(vals))
            assert not_stored == 0 or free > 0
            assert not t.last_error(reset=True)["bits"] & ~HANDOFF
        except shm.ShermanError as e:
            assert e.rc == shm.SHM_ENOMEM and not_stored, e
            error_state(t, shm.SHM_ENOMEM, NOMEM, NOMEM | HANDOFF)
        if not_stored == 0:
            assert t.stats()["pages_used"] == st["pages_used"]
            tall.check_contents(t, T, "the stored chunk again")
        T.close()
        T, kv, _ = truth(t, info, [])
        judge(kv)  # still before-or-after, whatever the second run added
    if more is not None:
        # a chunk that splits more leaves than pages are left
        st = t.stats()
        mk = more(st["pages_capacity"] - st["pages_used"] + 1)
        mv = mk ^ U64(0x6666)
        roomy = OracleTree(image=t.dump_image()[0], root_ptr=st["root_ptr"], spare_bytes=4 * ROOM)
        roomy.apply_batch(mk, mv)
        failed(lambda: t.insert_batch(dev(mk), dev(mv)), shm.SHM_ENOMEM)
        error_state(t, shm.SHM_ENOMEM, NOMEM, NOMEM | HANDOFF)
        T.close()
        T, kv2, _ = truth(t, info, [mk])
        am.classify_outcome(kv, contents(roomy), kv2, [])
        roomy.close()
        kv = kv2
    tk, tv = kv
    at = np.linspace(0, tk.size - 1, 24).astype(np.int64)
    ops = [(tk[at[0::3]], tv[at[0::3]] ^ U64(0x7777)),         # overwrites
           (tk[at[1::3]], np.zeros(8, dtype=U64))]             # deletes
    new = key_with_room(t, candidates[~np.isin(candidates, tk)])
    ops.append((new, new ^ U64(0x1357)))                        # a new key where there is room
    used = t.stats()["pages_used"]
    for k, v in ops:
        t.insert_batch(dev(k), dev(v))
        assert t.last_error()["bits"] == 0, t.last_error()
        T.apply_batch(k, v)
        gv, gf = gpu_search(t, k)
        assert np.array_equal(gf != 0, v != 0) and np.array_equal(gv[v != 0], v[v != 0])
    assert t.stats()["pages_used"] == used
    tall.check_contents(t, T, "the handle afterwards")
    T.close()


def after_failure(t, info, before, after, chunk, must_apply, monkeypatch, same_again,
                  more, candidates, force=0, trusted=True):
    """Everything asserted of a tree whose last chunk returned SHM_ENOMEM;
    returns classify_outcome's counts."""
    error_state(t, shm.SHM_ENOMEM, NOMEM, NOMEM | HANDOFF)
    T, kv, probe = truth(t, info, [before[0], after[0], chunk[0][chunk[0] != U64(KEY_MAX)]])
    got = am.classify_outcome(before, after, kv, must_apply)
    st = t.stats()
    print(f"failed chunk: {got}, pages free {st['pages_capacity'] - st['pages_used']}")
    # the table as the chunk's upkeep left it, before any search can rebuild it
    print(f"table trusted {t.vt_stats()['trusted']}, directory exact {t.dir_stats()['exact']}")
    table_clean(t, kv, trusted)
    readers(t, T, info, probe, "after the failed chunk", monkeypatch)
    handle_afterwards(t, T, kv, info, chunk, got["new_not_stored"], same_again, more,
                      candidates, force,
                      lambda now: am.classify_outcome(before, after, now, must_apply))
    return got


# ---- A: exact arenas from the built image --------------------------------------
def image(path):
    return tall.tall(2, path, True)


def exact_arena(path, spare):
    """the image in an arena with `spare` free pages, its table trusted and
    its directory exact and kept by every chunk"""
    img, root, info = image(path)
    t = shm.Tree(arena_bytes=img.nbytes + spare * PAGE, max_batch=tall.MAX_BATCH)
    t.load_image(img, root)
    st = t.stats()
    assert st["pages_capacity"] - st["pages_used"] == spare, st
    t.dir_config(maint="always")
    for _ in range(8):
        gpu_search(t, info["keys"][:512])
        if t.vt_stats()["trusted"] and t.dir_stats()["exact"]:
            break
    assert t.vt_stats()["trusted"] and t.dir_stats()["exact"], (t.vt_stats(), t.dir_stats())
    return t, info


@functools.lru_cache(maxsize=None)
def control(mode, path):
    """need (the pages the hot chunk takes in this mode, with room) and the
    oracle's contents without and with the chunk"""
    t, orc, info = tall.load(2, path, True)
    before = contents(orc)
    used = t.stats()["pages_used"]
    tall.apply_hot_chunk(t, orc, info, mode, grows=True)
    need = t.stats()["pages_used"] - used
    after = contents(orc)
    orc.close()
    t.close()
    assert need >= info["root_level"] + 2, need
    assert need <= SPARES[-1], f"the sweep stops at {SPARES[-1]} spare pages, need is {need}"
    return need, before, after


def thin_lows(info):
    low = info["leaf_lo"]
    thin = np.nonzero((info["leaf_live"] == 2) & (low != U64(info["hot_lo"])))[0]
    return low[thin[1:]]  # (not the first leaf: its lowest fence is key 0)


def split_thin_leaves(info, n):
    """60 absent keys in each of n thin leaves: each splits (2 + 60 > 53)"""
    low = thin_lows(info)
    pick = low[np.linspace(3, low.size - 3, n).astype(np.int64)]
    assert np.unique(pick).size == n
    return (pick[:, None] + U64(info["step"] // 64) * np.arange(1, 61, dtype=U64)[None, :]).ravel()


def unsplit_leaf_keeps_its_side_state(t, info, new, side0):
    """After the failed hot chunk: where the hot leaf's split did not fit (the
    leaf still covers its range and holds none of the new keys), its summary
    line and its occupancy bound are byte for byte those of before the chunk;
    and every page the failed take lost (below next_page, reached from
    nowhere) is untagged."""
    lines0, hw0, _ = side0
    img, root = t.dump_image()
    lines, hw, si = t.side_dump()
    pg = img.reshape(-1, PAGE)
    p = info["hot_page"]
    held = sm._slots(pg[p:p + 1])
    stored = np.isin(new, held[0][0][held[1][0] != 0])
    unsplit = not stored.any() and \
        sm._f64(pg[p:p + 1], sm.OFF_HIGHEST)[0] == U64(info["hot_hi"]) and pg[p, sm.OFF_LEVEL] == 0
    lost = np.nonzero(~sm.reached_pages(img, root)[1:])[0] + 1
    print(f"hot leaf {'unsplit' if unsplit else 'split'}, pages lost to the take: {lost.tolist()}")
    if unsplit:
        assert np.array_equal(lines[p], lines0[p]) and hw[p] == hw0[p], \
            (p, lines[p].tolist(), lines0[p].tolist(), int(hw[p]), int(hw0[p]))
    assert not (lines[lost, sm.SUM_OFF_TAG] == sm.SUM_LEAF).any(), lost


CASES_A = [(m, "middle") for m in tall.MODES] + [("default", "left"), ("default", "right")]


@pytest.mark.parametrize("spare", SPARES)
@pytest.mark.parametrize("mode,path", CASES_A)
def test_exact_arena(lib_ok, monkeypatch, mode, path, spare):
    """The hot chunk in an arena with `spare` free pages.  spare >= need: it
    succeeds, at need with the arena exactly full.  Below: SHM_ENOMEM, a tree
    both checkers accept, contents that are before-or-after per key with
    every op outside the hot leaf applied, every reader equal to the oracle
    on the dumped image, and a handle that goes on working."""
    need, before, after = control(mode, path)
    t, info = exact_arena(path, spare)
    keys, vals = am.hot_chunk(info)
    new = keys[(keys >= U64(info["hot_lo"])) & (keys < U64(info["hot_hi"]))]
    # the bug this guards against needs the table to answer for the new keys
    cls = get_paths.classify(new, t.vt_dump(), t.dir_dump(), {"exact": True})
    assert (cls == get_paths.TABLE).any(), cls
    if spare >= need:
        img, root, _ = image(path)
        orc = OracleTree(image=img, root_ptr=root, spare_bytes=ROOM)
        tall.apply_hot_chunk(t, orc, info, mode, grows=True)
        st = t.stats()
        assert st["pages_capacity"] - st["pages_used"] == spare - need, (st, need)
        assert t.dir_stats()["exact"], t.dir_stats()
        table_clean(t, contents(orc), True)
        tall.check_reads(t, orc, info, "the chunk fitted")
        orc.close()
        t.close()
        return
    assert shm._hooks().shm__upper_force(t.h, tall.MODES[mode]) == 0
    side0 = t.side_dump()
    failed(lambda: t.insert_batch(dev(keys), dev(vals)), shm.SHM_ENOMEM)
    unsplit_leaf_keeps_its_side_state(t, info, new, side0)
    outside = keys[(keys < U64(info["hot_lo"])) | (keys >= U64(info["hot_hi"]))]
    got = after_failure(t, info, before, after, (keys, vals), outside, monkeypatch,
                        same_again=True, more=lambda n: split_thin_leaves(info, n),
                        candidates=thin_lows(info)[1::7] + U64(info["step"] // 64),
                        force=tall.MODES[mode])
    assert got["applied"] >= 20  # the deletes and overwrites outside the hot leaf
    t.close()


def test_queued_search_after_a_failing_chunk(lib_ok):
    """The failing chunk and a search queued with no host call in between:
    the host learns of SHM_ENOMEM only at the synchronize, after the gets
    were queued, and they still answer what the pages hold."""
    _, before, after = control("default", "middle")
    t, info = exact_arena("middle", 0)
    keys, vals = am.hot_chunk(info)
    probe = tall.probes(info, np.unique(np.concatenate([before[0], after[0]])))
    dk, dv, dp = dev(keys), dev(vals), dev(probe)
    gv = torch.empty_like(dp)
    gf = torch.empty(dp.numel(), dtype=torch.uint8, device="cuda")
    t.insert_batch_async(dk, dv)
    t.search_batch(dp, gv, gf)
    failed(t.synchronize, shm.SHM_ENOMEM)
    error_state(t, shm.SHM_ENOMEM, NOMEM, NOMEM | HANDOFF)
    T, kv, probe2 = truth(t, info, [before[0], after[0]])
    assert np.array_equal(probe, probe2)
    am.classify_outcome(before, after, kv, keys[(keys < U64(info["hot_lo"])) |
                                                (keys >= U64(info["hot_hi"]))])
    assert_same(probe, *T.search_batch(probe), host(gv), gf.cpu().numpy(), "queued search")
    table_clean(t, kv, True)
    T.close()
    t.close()


# ---- B: arenas filled by inserts -------------------------------------------------
def gen_keys(t, first, n):
    k = gpu_helpers.gen_keys(t, first, n)
    return k[(k != U64(KEY_MAX)) & (k != U64(0))]


def flat_info(keys, around):
    """check_reads' description of a tree that came from inserts: no path
    pages, no deleted slots, the scans' windows around `around`"""
    step = ((1 << 64) // (keys.size + 2)) & ~63
    lo = int(np.median(around))
    return {"path": {}, "deleted": np.zeros(0, dtype=U64), "step": step,
            "hot_lo": lo, "hot_hi": min(lo + 54 * step, KEY_MAX - 1)}


def test_three_page_arena_is_refused(lib_ok):
    failed(lambda: shm.Tree(arena_bytes=3 * PAGE, max_batch=4096), shm.SHM_EINVAL)


@pytest.mark.parametrize("pages,chunk", [(4, 20), (64, 512)])
def test_arena_filled_by_inserts(lib_ok, monkeypatch, pages, chunk):
    """Chunks of hashed keys, a read phase between them, until the arena is
    full: many early splits race for the last pages, failed takes among
    them.  (4 pages, the documented minimum: 40 keys, then 20 at a time; the
    chunk that splits the root leaf needs the two free pages and gets them.)"""
    t = shm.Tree(arena_bytes=pages * PAGE, max_batch=4096)
    t.dir_config(maint="always")
    assert t.stats()["pages_capacity"] == pages - 1 and t.stats()["pages_used"] == 1
    orc = OracleTree(1 << 24)
    first, held, grown_full = 1, np.zeros(0, dtype=U64), False
    while True:
        assert first < 64 * pages, "the arena never ran out"
        n = 40 if first == 1 and pages == 4 else chunk
        k = gen_keys(t, first, n)
        v = k ^ U64(0x1111)
        first += n
        before = contents(orc)
        orc.apply_batch(k, v)
        try:
            t.insert_batch(dev(k), dev(v))
        except shm.ShermanError as e:
            assert e.rc == shm.SHM_ENOMEM, e
            break
        assert t.last_error()["bits"] == 0, t.last_error()
        st = t.stats()
        grown_full |= st["root_level"] == 1 and st["pages_used"] == st["pages_capacity"]
        held = np.concatenate([held, k])
        for _ in range(6):
            gpu_search(t, held[-512:])
    after = contents(orc)
    orc.close()
    if pages == 4:
        # the root leaf split into the last two pages, and that chunk succeeded
        assert grown_full and t.stats()["root_level"] == 1, t.stats()
    info = flat_info(after[0], k)
    cand = gen_keys(t, 1 << 20, 256)
    got = after_failure(t, info, before, after, (k, v), [], monkeypatch, same_again=False,
                        more=None, candidates=cand)
    assert got["new_not_stored"] > 0
    print(f"arena of {pages} pages: the failing chunk of {k.size} new keys stored "
          f"{got['new_stored']}, left {got['new_not_stored']}")
    t.close()


# ---- C: a rejected chunk beside a trusted table ----------------------------------
def test_rejected_chunk_beside_a_trusted_table(lib_ok):
    """A chunk holding kKeyMax next to new keys and overwrites, queued behind
    nothing and in front of a search: SHM_EINVAL, and no reader sees any of
    it -- the table and the directory took nothing from the rejected ops."""
    t = shm.Tree(arena_bytes=32 << 20, max_batch=4096)
    t.dir_config(maint="always")
    orc = OracleTree(1 << 24)
    base = gen_keys(t, 1, 4000)
    bv = base ^ U64(0x1111)
    t.insert_batch(dev(base), dev(bv))
    orc.apply_batch(base, bv)
    for _ in range(8):
        gpu_search(t, base[:512])
        if t.vt_stats()["trusted"] and t.dir_stats()["exact"]:
            break
    assert t.vt_stats()["trusted"] and t.dir_stats()["exact"], (t.vt_stats(), t.dir_stats())
    new = gen_keys(t, 1 << 20, 200)
    over = base[::40]
    keys = np.concatenate([new[:100], over, np.array([KEY_MAX], dtype=U64), new[100:]])
    vals = keys ^ U64(0x9999)
    cls = get_paths.classify(np.concatenate([new, over]), t.vt_dump(), t.dir_dump(),
                             {"exact": True})
    assert (cls == get_paths.TABLE).any(), cls
    info = flat_info(base, new)
    probe = tall.probes(info, np.unique(np.concatenate([base, new])))
    dk, dv, dp = dev(keys), dev(vals), dev(probe)
    gv = torch.empty_like(dp)
    gf = torch.empty(dp.numel(), dtype=torch.uint8, device="cuda")
    t.insert_batch_async(dk, dv)
    t.search_batch(dp, gv, gf)
    failed(t.synchronize, shm.SHM_EINVAL)
    e = t.last_error(reset=True)
    assert e["bits"] == KEYMAX_BIT and e["status"] == shm.SHM_EINVAL, e
    want = orc.search_batch(probe)
    assert not want[1][np.isin(probe, new)].any()
    assert_same(probe, *want, host(gv), gf.cpu().numpy(), "queued search")
    T, kv, _ = truth(t, info, [new])
    assert np.array_equal(kv[0], contents(orc)[0]) and np.array_equal(kv[1], contents(orc)[1])
    table_clean(t, kv, True)
    tall.check_reads(t, orc, info, "after the rejected chunk")
    tall.enter_read_phase(t, probe)
    tall.check_reads(t, orc, info, "after the rejected chunk, read phase")
    T.close()
    orc.close()
    t.close()
