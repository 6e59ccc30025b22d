"""Descending scans with a count limit (shm_rscan_batch, Tree.rscan_batch /
floor_batch) on the GPU against the numpy model (tests/rscan_model.py).

Built like tests/test_gpu_scan.py: every check compares counts, keys and
values exactly with the model, asserts that the words of a scan's row past its
count still hold the sentinel the buffers were filled with, that status is
[77, 0] and that the device error bits are zero.  The trees are the smallest
on which each path of the kernel exists: the step to the left through the
directory and from the root, over leaves with holes, over leaves with no valid
entry, across a stale directory and a missing separator, on trees of height 4
and 8, and across more leaves than one descent's hop bound allows.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena_model as am  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, host, lib_ok, SENT, U64  # noqa: E402
import test_gpu_arena_full as full  # noqa: E402
import test_gpu_tall as tall  # noqa: E402
from oracle.pyoracle import OracleTree, to_key  # noqa: E402
from rscan_model import KEY_MAX, RScanModel  # noqa: E402

ARENA = 64 << 20
TOP = 1 << 63


def hashed_keys(lo, hi):
    return np.array([to_key(i) for i in range(lo, hi)], dtype=U64)


def u64(*xs):
    return np.array([int(x) for x in xs], dtype=U64)


def put(t, orc, keys, vals):
    """One batch into both trees (value 0 deletes)."""
    t.insert_batch(dev(keys), dev(vals))
    orc.apply_batch(keys, vals)


def queue_rscans(t, start, limit, stop=None):
    """Queues the scans into sentinel-filled buffers; returns what
    check_rscans needs.  status[0] is set to a mark the call must leave
    alone."""
    n = start.size
    keys = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
    vals = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
    counts = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    status = torch.tensor([77, 0], dtype=torch.int64, device="cuda")
    d_hi = dev(start)
    d_lo = None if stop is None else dev(stop)
    pend = t.rscan_batch(d_hi, limit, lo=d_lo, keys=keys, vals=vals, counts=counts, status=status)
    return pend, status, (d_hi, d_lo)


def check_rscans(model, queued, start, limit, stop=None):
    pend, status, _ = queued
    c, k, v = pend.result()
    assert status.cpu().tolist() == [77, 0], status
    c, k, v = c.cpu().numpy(), host(k), host(v)
    mc, mk, mv, w = model.scan(start, limit, stop)
    bad = np.nonzero(c != mc)[0]
    assert bad.size == 0, (f"{bad.size} counts differ, first: scan {bad[0]} "
                           f"start={int(start[bad[0]]):#x} limit={limit} gpu={c[bad[0]]} "
                           f"model={mc[bad[0]]}")
    assert k.shape == mk.shape == (start.size, limit)
    for name, g, m in (("key", k, mk), ("value", v, mv)):
        ne = np.argwhere(w & (g != m))
        assert ne.size == 0, (f"{name}s differ at {len(ne)} places, first: scan {ne[0][0]} "
                              f"start={int(start[ne[0][0]]):#x} limit={limit} pos {ne[0][1]} "
                              f"gpu={int(g[tuple(ne[0])]):#x} model={int(m[tuple(ne[0])]):#x}")
        assert (g[~w] == U64(SENT)).all(), f"{name} row tails were written (limit {limit})"
    return mc, mk, mv


def rscan_and_check(t, model, start, limit, stop=None):
    start = np.ascontiguousarray(start, dtype=U64)
    if stop is not None:
        stop = np.ascontiguousarray(stop, dtype=U64)
    out = check_rscans(model, queue_rscans(t, start, limit, stop), start, limit, stop)
    assert t.last_error()["bits"] == 0, t.last_error()
    return out


def whole_tree(t, model, n_scans=1):
    """Scans from KEY_MAX with room for one pair more than the tree holds:
    the sorted contents reversed."""
    n = model.keys.size
    start = np.full(n_scans, KEY_MAX, dtype=U64)
    mc, mk, mv = rscan_and_check(t, model, start, n + 1)
    assert (mc == n).all()
    for i in range(n_scans):
        assert np.array_equal(mk[i, :n], model.keys[::-1])
        assert np.array_equal(mv[i, :n], model.vals[::-1])


def starts_around(model):
    """Every 37th stored key, those keys +- 1, 0, below the minimum, above the
    maximum, KEY_MAX - 1 and KEY_MAX."""
    s = model.keys[::37]
    return np.concatenate([s, s + U64(1), s - U64(1),
                           u64(0, int(model.keys[0]) - 1, int(model.keys[-1]) + 1,
                               KEY_MAX - 1, KEY_MAX)])


# ---- 1: a churned tree -------------------------------------------------------------
@pytest.mark.parametrize("leaf_dir", [True, False])
def test_churned_tree_against_the_model(lib_ok, leaf_dir):
    """20,000 hashed keys, then three rounds of deletes (value 0), overwrites
    and re-inserts, mirrored into the oracle: leaves with holes and with slots
    out of key order.  After each round every limit from every start."""
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 15, leaf_dir=leaf_dir)
    orc = OracleTree(ARENA)
    base = hashed_keys(1, 20001)
    put(t, orc, base, base ^ U64(0x1111))
    rng = np.random.default_rng(41)
    crossed = 0
    for r in range(3):
        live, _ = orc.dump()
        live = live[rng.permutation(live.size)]
        dele, over = live[:3000], live[3000:7000]
        put(t, orc, dele, np.zeros(dele.size, dtype=U64))
        put(t, orc, over, over ^ U64(0xABC0 + r))
        back = np.concatenate([dele[:1500], hashed_keys(30001 + 1500 * r, 31501 + 1500 * r)])
        put(t, orc, back, back ^ U64(0x7700 + r))
        model = RScanModel.of(orc)
        assert model.keys.size == t.check()["keys"]
        start = starts_around(model)
        for limit in (1, 2, 7, 53, 54, 55, 200):
            mc, mk, _ = rscan_and_check(t, model, start, limit)
            last = mk[np.arange(start.size), np.maximum(mc, 1) - 1]
            crossed += int(((mc > 0) & (start >= U64(TOP)) & (last < U64(TOP))).sum())
    assert (base < U64(TOP)).any() and (base >= U64(TOP)).any()
    assert crossed > 0, "no scan's result crossed 2^63 downward"
    orc.close()
    t.close()


# ---- 2: a dense tree ---------------------------------------------------------------
class Dense:
    """3,000 dense keys 3 * i (i = 1 .. 3000) inserted in a random permutation,
    then every fifth deleted: read-only after the build."""

    def __init__(self, leaf_dir):
        self.t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 12, leaf_dir=leaf_dir)
        self.orc = OracleTree(ARENA)
        rng = np.random.default_rng(43)
        ks = np.arange(1, 3001, dtype=U64) * U64(3)
        dele = ks[::5].copy()
        ks = ks[rng.permutation(ks.size)]
        for c in range(0, ks.size, 500):
            put(self.t, self.orc, ks[c:c + 500], ks[c:c + 500] + U64(7))
        put(self.t, self.orc, dele, np.zeros(dele.size, dtype=U64))
        self.model = RScanModel.of(self.orc)
        assert self.model.keys.size == 2400 == self.t.check()["keys"]


@pytest.fixture(scope="module", params=[True, False], ids=["dir", "nodir"])
def dense(request, lib_ok):
    d = Dense(request.param)
    yield d
    d.orc.close()
    d.t.close()


def test_every_alignment_against_leaf_ends(dense):
    """Start at every stored key and every key - 1, unbounded: the limit cut
    falls at each position inside a leaf and at each leaf boundary without
    the test knowing the fences."""
    s = dense.model.keys
    start = np.concatenate([s, s - U64(1)])
    for limit in (1, 54, 55, 108):
        rscan_and_check(dense.t, dense.model, start, limit)


def test_the_stop_bound(dense):
    t, model = dense.t, dense.model
    s = model.keys
    absent = s + U64(1)  # stored keys are multiples of 3
    i = np.arange(0, s.size - 80, 7)
    cases = [  # (start, stop, matches)
        (s[:-1], s[:-1] + U64(1), 0),                  # stop > start
        (s, s, 1),                                     # stop == start on a stored key
        (absent, absent, 0),                           # stop == start on an absent key
        (s[i + 5] + U64(1), s[i], 6),                  # stop on a stored key
        (s[i + 5] - U64(1), s[i] + U64(1), 4),         # stop between two stored keys
        (s[i + 70] + U64(1), s[i], 71),                # ends the scan before limit 108, leaves apart
        (s[i + 70], s[i] + U64(2), 70),
    ]
    for limit in (1, 54, 108):
        for start, stop, want in cases:
            mc, _, _ = rscan_and_check(t, model, start, limit, stop)
            assert (mc == min(want, limit)).all(), (limit, want)


# ---- 3: floor ----------------------------------------------------------------------
@pytest.mark.parametrize("leaf_dir", [True, False])
def test_floor_batch_against_searchsorted(lib_ok, leaf_dir):
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 15, leaf_dir=leaf_dir)
    base = hashed_keys(1, 20001)
    vals = base ^ U64(0x6666)
    t.insert_batch(dev(base), dev(vals))
    order = np.argsort(base)
    sk, sv = base[order], vals[order]
    probe = np.concatenate([sk[::3], sk[::5] + U64(1), sk[::7] - U64(1),
                            u64(int(sk[-1]) + 1, KEY_MAX - 1, KEY_MAX, 0, int(sk[0]) - 1)])
    found, k, v = t.floor_batch(dev(probe))
    found, k, v = found.cpu().numpy(), host(k), host(v)
    idx = np.searchsorted(sk, probe, side="right") - 1
    want = idx >= 0
    assert want[-5:-2].all() and not want[-2:].any()
    assert np.array_equal(found, want)
    assert np.array_equal(k[want], sk[idx[want]]) and np.array_equal(v[want], sv[idx[want]])
    assert (k[~want] == 0).all() and (v[~want] == 0).all()
    assert k[-3] == k[-4] == k[-5] == sk[-1]  # KEY_MAX, KEY_MAX - 1, maximum + 1: the maximum
    assert (probe >= U64(TOP)).any() and (k[want] < U64(TOP)).any()
    assert t.last_error()["bits"] == 0
    t.close()


# ---- 4: whole-tree scans over a stale directory --------------------------------------
def test_whole_tree_over_a_stale_directory(lib_ok):
    """2^16 hashed keys in two chunks, then 1,800 keys that split 60 leaves
    behind a directory that is not rebuilt (test_gpu_scan's stale tree, with
    its conditions).  Two scans from KEY_MAX return every pair, over the
    stale directory and again from the root without one: more than 2,000
    steps to the left each, of two hops each from the root, more than a hop
    count shared by all of a scan's descents (4,096) would allow."""
    t = shm.Tree(arena_bytes=256 << 20, max_batch=1 << 15, leaf_dir=True)
    orc = OracleTree(256 << 20)
    base = hashed_keys(1, (1 << 16) + 1)
    for c in (0, 1 << 15):
        put(t, orc, base[c:c + (1 << 15)], base[c:c + (1 << 15)] ^ U64(0x2222))
    rng = np.random.default_rng(47)
    probe = dev(base[rng.integers(0, base.size, 4096)])
    out = torch.empty_like(probe)
    for _ in range(5):
        t.search_batch(probe, out)
    t.synchronize()
    d0 = t.dir_stats()
    assert d0["builds"] >= 1 and d0["form"] != "none"
    t.dir_config(maint=False)
    pages0 = t.stats()["pages_used"]
    srt = np.sort(base)
    anchors = srt[rng.choice(srt.size - 1, 60, replace=False)]
    new = (anchors[:, None] + np.arange(1, 31, dtype=U64)[None, :]).ravel()
    assert np.intersect1d(new, base).size == 0 and np.unique(new).size == 1800
    put(t, orc, new, new ^ U64(0x3333))
    model = RScanModel.of(orc)
    assert model.keys.size == (1 << 16) + 1800
    leaves = t.check()["leaves"]
    assert leaves > 2048, leaves
    whole_tree(t, model, n_scans=2)
    start = np.concatenate([anchors - U64(1), anchors, anchors + U64(1), anchors + U64(31)])
    for limit in (1, 40, 120):
        rscan_and_check(t, model, start, limit)
    # the same pages without a directory: two hops per step from the root
    img, root = t.dump_image()
    no_dir = shm.Tree(arena_bytes=256 << 20, max_batch=1 << 15, leaf_dir=False)
    no_dir.load_image(img, root)
    assert 2 * leaves > 4096 and no_dir.stats()["root_level"] == 2
    whole_tree(no_dir, model, n_scans=2)
    no_dir.close()
    pages1 = t.stats()["pages_used"]
    d1 = t.dir_stats()
    print("stale directory: pages", pages0, "->", pages1, "leaves", leaves, d1)
    assert pages0 + 20 <= pages1 < pages0 + pages0 // 32, (pages0, pages1)
    assert d1["builds"] == d0["builds"], (d0, d1)
    orc.close()
    t.close()


# ---- 5: tall images ------------------------------------------------------------------
@pytest.mark.parametrize("leaf_dir", [True, False], ids=["dir", "nodir"])
@pytest.mark.parametrize("root_level,path", [(lvl, p) for lvl in (3, 7)
                                             for p in ("left", "middle", "right")])
def test_tall_images(lib_ok, root_level, path, leaf_dir):
    """Root levels 3 and 7: every step to the left is a descent of 4 or 8
    pages without the directory.  Every 17th thin leaf holds deleted entries
    only, so scans step over leaves that give nothing."""
    t, orc, info = tall.load(root_level, path, root_level < 7, leaf_dir=leaf_dir)
    model = RScanModel(info["keys"], info["vals"])
    assert np.array_equal(model.keys, info["keys"])
    fences = np.array([f for lvl in info["path"] for f in info["path"][lvl][1:]], dtype=U64)
    s = info["keys"]
    start = np.unique(np.concatenate([s, s + U64(1), s - U64(1), fences, fences + U64(1),
                                      fences - U64(1), u64(0, KEY_MAX)]))
    for limit in (1, 3, 60):
        rscan_and_check(t, model, start, limit)
    whole_tree(t, model)
    # from a deleted key: the previous live key, past the leaf that held it
    dead = info["deleted"]
    assert dead.size > 0
    mc, mk, _ = rscan_and_check(t, model, dead, 1)
    leaf = np.searchsorted(info["leaf_lo"], dead, side="right") - 1
    assert (info["leaf_live"][leaf] == 0).all()
    stepped = (mc == 1) & (mk[:, 0] < info["leaf_lo"][leaf])
    assert np.array_equal(stepped, mc == 1) and stepped.sum() > 0
    at = np.searchsorted(s, dead, side="left") - 1
    assert np.array_equal(mk[mc == 1, 0], s[at[at >= 0]])
    orc.close()
    t.close()


# ---- 6: entry states -----------------------------------------------------------------
@pytest.mark.parametrize("leaf_dir", [True, False], ids=["dir", "nodir"])
def test_entry_states(lib_ok, leaf_dir):
    """Deleted slots with stale key bytes, stale copies of live keys, torn
    entries, entries at version 15, and a last leaf with no valid entry."""
    img, root, info = ib.build_entry_states()
    orc = OracleTree(image=img, root_ptr=root, spare_bytes=1 << 20)
    rc, _ = orc.check()
    assert rc == 0, rc
    orc.close()
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 14, leaf_dir=leaf_dir)
    t.load_image(img, root)
    model = RScanModel(info["keys"], info["vals"])
    n = info["n_valid"]
    assert model.keys.size == n
    # from KEY_MAX: over the all-deleted last leaf to the largest valid key
    assert info["keys"][-1] < info["leaf_lo"][-1]
    mc, mk, _ = rscan_and_check(t, model, u64(KEY_MAX, KEY_MAX - 1), 1)
    assert mc.tolist() == [1, 1] and (mk[:, 0] == info["keys"][-1]).all()
    mc, mk, mv = rscan_and_check(t, model, u64(KEY_MAX), n + 1)
    got = mk[0, :n]
    assert mc[0] == n and np.array_equal(got, info["keys"][::-1])
    assert np.array_equal(mv[0, :n], info["vals"][::-1])
    assert not np.isin(got, info["torn"]).any() and not np.isin(got, info["deleted"]).any()
    for k in info["stale_copy"]:
        assert int((got == k).sum()) == 1, hex(int(k))
    assert info["v15_keys"].size > 0 and np.isin(info["v15_keys"], got).all()
    every = np.concatenate([info["keys"], info["torn"], info["deleted"], info["stale_copy"]])
    start = np.unique(np.concatenate([every, every + U64(1), every - U64(1), info["leaf_lo"],
                                      info["leaf_lo"] - U64(1), u64(0, KEY_MAX - 1, KEY_MAX)]))
    bad = np.concatenate([info["torn"], info["deleted"]])
    for limit in (1, 21, 60):
        mc, mk, _ = rscan_and_check(t, model, start, limit)
        w = np.arange(limit)[None, :] < mc[:, None]
        assert not np.isin(mk[w], bad).any()
    t.close()


# ---- 7: the B-link state after SHM_ENOMEM ----------------------------------------------
def test_new_leaves_without_a_separator(lib_ok):
    """The level-2 image in arenas with too few spare pages for the hot
    chunk: where the leaf level fitted and an internal level did not, the new
    leaves hang on their left sibling alone.  A step to the left lands on the
    old leaf and turns right to them."""
    need, _, _ = full.control("default", "middle")
    assert need >= 3, need
    hung = 0
    for spare in range(1, need):
        t, info = full.exact_arena("middle", spare)
        leaves0 = t.check()["leaves"]
        keys, vals = am.hot_chunk(info)
        try:
            t.insert_batch(dev(keys), dev(vals))
            nomem = False
        except shm.ShermanError as e:
            assert e.rc == shm.SHM_ENOMEM, e
            nomem = True
            full.error_state(t, shm.SHM_ENOMEM, full.NOMEM, full.NOMEM | full.HANDOFF)
        assert nomem, (spare, need)
        img, root = t.dump_image()
        T = OracleTree(image=img, root_ptr=root)
        rc, shape = T.check()
        assert rc == 0, rc
        grew = shape["leaves"] > leaves0
        assert t.check()["leaves"] == shape["leaves"]
        hung += int(grew)
        model = RScanModel.of(T)
        T.close()
        hot_lo, hot_hi = info["hot_lo"], info["hot_hi"]
        k = model.keys
        inside = k[(k >= U64(hot_lo)) & (k < U64(hot_hi))]
        above = k[np.searchsorted(k, U64(hot_hi)):][:4]
        start = np.unique(np.concatenate([inside, inside + U64(1), inside - U64(1), above,
                                          above - U64(1), above + U64(1),
                                          u64(hot_lo, hot_lo - 1, hot_lo + 1, hot_hi, hot_hi - 1,
                                              hot_hi + 1)]))
        no_dir = shm.Tree(arena_bytes=img.nbytes + 4 * full.PAGE, max_batch=tall.MAX_BATCH,
                          leaf_dir=False)
        no_dir.load_image(img, root)
        for tree in (t, no_dir):
            whole_tree(tree, model)
            for limit in (1, 60):
                rscan_and_check(tree, model, start, limit)
        print(f"spare {spare} of {need}: leaves {leaves0} -> {shape['leaves']}")
        no_dir.close()
        t.close()
    assert hung > 0, "no arena left new leaves without a separator"


# ---- 8: edge cases and ordering ----------------------------------------------------------
@pytest.mark.parametrize("leaf_dir", [True, False])
def test_empty_tree_and_empty_batch(lib_ok, leaf_dir):
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 12, leaf_dir=leaf_dir)
    model = RScanModel(np.zeros(0, dtype=U64), np.zeros(0, dtype=U64))
    start = u64(0, 1, 12345, TOP, KEY_MAX - 1, KEY_MAX)
    for limit in (1, 60):
        mc, _, _ = rscan_and_check(t, model, start, limit)
        assert (mc == 0).all()
        rscan_and_check(t, model, start, limit, stop=np.zeros(start.size, dtype=U64))
    # n == 0: SHM_OK (no exception), nothing launched, nothing written
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    keys = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    vals = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    counts = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    status = torch.tensor([77, 0], dtype=torch.int64, device="cuda")
    c, k, v = t.rscan_batch(e, 4, keys=keys, vals=vals, counts=counts, status=status).result()
    assert c.numel() == 0 and tuple(k.shape) == (0, 4) and tuple(v.shape) == (0, 4)
    assert status.cpu().tolist() == [77, 0]
    for b in (keys, vals, counts):
        assert (host(b) == U64(SENT)).all()
    c, k, v = t.rscan_batch(e, 3, lo=e).result()
    assert c.numel() == 0
    found, k1, v1 = t.floor_batch(e)
    assert found.numel() == k1.numel() == v1.numel() == 0
    assert t.last_error()["bits"] == 0
    t.close()


@pytest.mark.parametrize("leaf_dir", [True, False])
def test_stream_order(lib_ok, leaf_dir):
    """rscan, insert_batch_async of keys inside the scans' windows, rscan, all
    queued on one stream with no wait between them: the first scan sees the
    tree before the insert, the second the tree after it."""
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 15, leaf_dir=leaf_dir)
    orc = OracleTree(ARENA)
    base = hashed_keys(1, 20001)
    put(t, orc, base, base ^ U64(0x4444))
    before = RScanModel.of(orc)
    start = before.keys[30::61].copy()
    ins = np.concatenate([start - U64(1), start - U64(2), before.keys[25::61]])  # new keys, overwrites
    iv = ins ^ U64(0x5555)
    limit = 20
    s = torch.cuda.current_stream()
    q1 = queue_rscans(t, start, limit)
    dk, dv = dev(ins), dev(iv)
    t.insert_batch_async(dk, dv, stream=s)
    q2 = queue_rscans(t, start, limit)
    orc.apply_batch(ins, iv)
    after = RScanModel.of(orc)
    _, k1, _ = check_rscans(before, q1, start, limit)
    _, k2, _ = check_rscans(after, q2, start, limit)
    assert not np.array_equal(k1, k2)  # the insert lies inside the windows
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


def test_status_accumulates_only_error_bits(lib_ok):
    """One status pair passed to three calls: status[0] is never written, and
    status[1] is ORed into (a bit set by the caller stays, clean scans add
    none)."""
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 12)
    base = hashed_keys(1, 2001)
    t.insert_batch(dev(base), dev(base ^ U64(0x1234)))
    mark = 1 << 40
    status = torch.tensor([77, mark], dtype=torch.int64, device="cuda")
    start = dev(np.sort(base)[::17])
    got = []
    for limit in (1, 9, 70):
        c, k, v = t.rscan_batch(start, limit, status=status).result()
        got.append(int(c.sum().item()))
        assert status.cpu().tolist() == [77, mark]
    assert got[0] == start.numel() and got[0] < got[1] < got[2]
    assert t.last_error()["bits"] == 0
    t.close()
