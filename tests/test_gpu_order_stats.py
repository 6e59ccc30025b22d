"""Order statistics on the GPU (Tree.rank_batch / count_batch / select_batch /
quantile_keys -> shm_rank_batch / shm_count_batch / shm_select_batch ->
order.hip over the order index of tree_order.cpp).

Expected results come from tests/export_model.py on the tree's own
dump_image() (a numpy walk sharing no code with the library): with K, V its
export, a key's rank is np.searchsorted(K, k, "left"), position r holds
(K[r], V[r]) and a range's count is the difference of two ranks.
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
import export_model as em  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, host, lib_ok, SENT, U64  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

KEY_MAX = (1 << 64) - 1
PAGE = 1024
ARENA = 64 << 20
MAX_BATCH = 1 << 14
EDGE = 40      # the first and last keys / ranks that a strided query set keeps
DENSE = 300    # up to here every key / rank is queried


def tree(**kw):
    return shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, **kw)


def sentinels(n, dtype=torch.int64):
    return torch.full((n,), SENT if dtype == torch.int64 else 0x5A, dtype=dtype, device="cuda")


def model_of(t):
    img, root = t.dump_image()
    k, v = em.export(img, root, node_id=t.node_id)
    return k, v, img


def builds(t):
    return t.order_stats()["builds"]


def thin(a):
    """every element up to DENSE of them, else the first and last EDGE and a
    stride between"""
    if a.size <= DENSE:
        return a
    mid = a[EDGE:-EDGE]
    return np.concatenate([a[:EDGE], mid[::mid.size // 200 + 1], a[-EDGE:]])


def key_points(K, extra=()):
    """every stored key (thinned) and the extra keys, their neighbours +-1
    (wrapping: any u64 is a key to ask for), and the ends of the key space"""
    k = np.concatenate([thin(K), np.asarray(extra, dtype=U64)])
    ends = np.array([0, 1, KEY_MAX - 1, KEY_MAX], dtype=U64)
    return np.unique(np.concatenate([k, k + U64(1), k - U64(1), ends]))


def rank_points(n):
    r = thin(np.arange(n + 2, dtype=U64))
    return np.concatenate([r, np.array([1 << 63, KEY_MAX], dtype=U64)])


def range_points(P, seed):
    """(from, to) drawn from the points: random pairs (half of them from > to),
    neighbours, from == to, and the whole key space"""
    rng = np.random.default_rng(seed)
    m = 2 * P.size
    lo = np.concatenate([P[rng.integers(0, P.size, m)], P[:-1], P, P[1:],
                         np.array([0, KEY_MAX, 0], dtype=U64)])
    hi = np.concatenate([P[rng.integers(0, P.size, m)], P[1:], P, P[:-1],
                         np.array([KEY_MAX, KEY_MAX, 0], dtype=U64)])
    assert lo.dtype == U64 and hi.dtype == U64
    return lo, hi


def want_counts(K, lo, hi):
    """rank(to + 1) - rank(from); no stored key equals KEY_MAX, so the keys
    <= to are the keys below to + 1 also for to == KEY_MAX"""
    c = np.searchsorted(K, hi, "right").astype(np.int64) - np.searchsorted(K, lo, "left")
    return np.where(lo <= hi, c, 0).astype(U64)


def first_bad(got, want, arg):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else (bad.size, hex(int(arg[bad[0]])), int(got[bad[0]]),
                                       int(want[bad[0]]))


def check_order(t, K, V, extra=(), seed=0, what=""):
    """rank, select and count of the query sets above equal the model (K, V);
    no error bit, in the calls' status words or on the handle"""
    N = K.size
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    P = key_points(K, extra)
    got = host(t.rank_batch(dev(P), status=st))
    assert first_bad(got, np.searchsorted(K, P, "left").astype(U64), P) is None, \
        (what, "rank", first_bad(got, np.searchsorted(K, P, "left").astype(U64), P))
    R = rank_points(N)
    k, v, f = t.select_batch(dev(R), status=st)
    inside = R < U64(N)
    at = np.minimum(R, U64(max(N, 1) - 1)).astype(np.int64)
    wk = np.where(inside, K[at] if N else U64(0), U64(KEY_MAX))
    wv = np.where(inside, V[at] if N else U64(0), U64(0))
    assert np.array_equal(f.cpu().numpy(), inside.astype(np.uint8)), (what, "found")
    assert first_bad(host(k), wk, R) is None, (what, "select key", first_bad(host(k), wk, R))
    assert first_bad(host(v), wv, R) is None, (what, "select value", first_bad(host(v), wv, R))
    lo, hi = range_points(P, seed)
    got = host(t.count_batch(dev(lo), dev(hi), status=st))
    want = want_counts(K, lo, hi)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, "count", bad.size, hex(int(lo[bad[0]])), hex(int(hi[bad[0]])),
                           int(got[bad[0]]), int(want[bad[0]]))
    t.synchronize()
    assert host(st).tolist() == [0, 0], (what, host(st))
    assert t.last_error()["bits"] == 0, (what, t.last_error())
    return lo, hi, want


def leaf_fences(img):
    """the fence keys of every leaf page of an image (reached or not: they are
    only keys to ask for)"""
    pg = np.asarray(img, dtype=np.uint8).reshape(-1, PAGE)[1:]
    leaf = (np.ascontiguousarray(pg[:, 9:17]).view("<u8").reshape(-1) == 0) & (pg[:, 25] == 0)
    f = np.ascontiguousarray(pg[leaf][:, 28:44]).view("<u8").reshape(-1).astype(U64)
    return np.unique(f)


@functools.lru_cache(maxsize=None)
def entry_states():
    img, root, info = ib.build_entry_states()
    img.setflags(write=False)
    return img, root, info


# ---- 1. the number of units at the search levels' boundaries -------------------------

@pytest.fixture(scope="module")
def wide_tree(lib_ok):
    # 65,537 leaves and the 1,095 pages above them: 65 MB of pages
    t = shm.Tree(arena_bytes=128 << 20, max_batch=MAX_BATCH)
    yield t
    t.close()


UNIT_CASES = [tuple(range(1, 71))] + [(u,) for u in (255, 256, 257, 258, 4095, 4096, 4097, 4098,
                                                      65535, 65536, 65537)]


@pytest.mark.parametrize("units", UNIT_CASES, ids=lambda u: f"{u[0]}-{u[-1]}")
def test_unit_counts_at_the_level_boundaries(wide_tree, units):
    """bulk_load(leaf_fill = 1) makes U leaves of one key each, so U units: at
    every U around a power of a fan-out up to 256 the search levels gain a
    word, a block or a level."""
    t = wide_tree
    for U in units:
        keys = bm.shape_keys(U, "spread", seed=U)
        vals = bm.shape_vals(keys)
        t.bulk_load(dev(keys), dev(vals), 1, 60)
        K, V, _ = model_of(t)
        assert np.array_equal(K, keys) and np.array_equal(V, vals)
        b = builds(t)
        check_order(t, K, V, seed=U, what=U)
        st = t.order_stats()
        assert (st["units"], st["pairs"], st["builds"]) == (U, U, b + 1), (U, st)


def test_the_empty_tree(lib_ok):
    t = tree()
    none = np.zeros(0, dtype=U64)
    check_order(t, none, none, what="created")
    st = t.order_stats()
    assert (st["units"], st["pairs"], st["builds"]) == (1, 0, 1) and st["bytes"] > 0
    assert st["last_build_ms"] >= 0
    t.close()


# ---- 2. inside a leaf ----------------------------------------------------------------

@pytest.mark.parametrize("n,lf,inf", bm.SHAPES)
def test_loaded_shapes(lib_ok, n, lf, inf):
    """the empty tree, one key, leaves of 53 and of 54 candidates, exactly full
    pages, root levels 0..7; every fence key and its neighbours"""
    keys = bm.shape_keys(n, bm.shape_kind(n, lf, inf))
    vals = bm.shape_vals(keys)
    t = tree()
    t.bulk_load(dev(keys), dev(vals), lf, inf)
    K, V, img = model_of(t)
    assert np.array_equal(K, keys)
    check_order(t, K, V, extra=thin(leaf_fences(img)), seed=n, what=(n, lf, inf))
    t.close()


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
def test_images(lib_ok, name, make):
    """Pages in shuffled order, a 53-entry leaf in shuffled slots, leaves whose
    entries are all deleted (build_tall); deleted, torn and null entries, holes
    and a last leaf with no valid entry (build_entry_states); and that image
    with the last separator of the root and / or of every level-1 page
    dropped, so that leaves and level-1 pages hang on their left sibling
    alone.  count_batch also equals range_query's counts."""
    img, root, info = make()
    t = tree()
    t.load_image(img, root)
    K, V = em.export(img, root)
    assert np.array_equal(K, info["keys"]) and np.array_equal(V, info["vals"])
    lo, hi, want = check_order(t, K, V, extra=thin(leaf_fences(img)), seed=3, what=name)
    assert_counts_equal_range_query(t, lo, hi, want, name)
    t.close()


def assert_counts_equal_range_query(t, lo, hi, want, what):
    lo_d, hi_d = dev(lo), dev(hi)
    c = sentinels(lo.size)
    rc = shm.lib().shm_range_query(t.h, shm._ptr(lo_d), shm._ptr(hi_d), lo.size, shm._ptr(c), None,
                                   None, None)
    assert rc == shm.SHM_OK
    t.synchronize()
    assert np.array_equal(host(c), want), what


# ---- 3. chains -----------------------------------------------------------------------

def test_after_the_arena_ran_out(lib_ok):
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
    K, V, img = model_of(t)
    assert K.size > 512
    lo, hi, want = check_order(t, K, V, extra=leaf_fences(img), seed=4, what="arena full")
    assert_counts_equal_range_query(t, lo, hi, want, "arena full")
    t.close()


# ---- 4. pages the tree does not reach ------------------------------------------------

@pytest.mark.parametrize("which", ["tall", "entry_states"])
def test_unreached_pages_are_not_read(lib_ok, which):
    """The image with six soil pages of every kind behind it: results equal
    the model over the pages the root reaches, and no selected value is a soil
    value."""
    if which == "tall":
        img, root, info = ib.build_tall(2, "middle", True)
    else:
        img, root, info = entry_states()
    pages, soil = ib.soil_pages(6, ib.soil_keys(info, hint=(0, 64)), seed=1,
                                first_page=img.size // PAGE)
    both = ib.with_soil(img, pages)
    t = shm.Tree(arena_bytes=both.nbytes + 64 * PAGE, max_batch=MAX_BATCH)
    t.load_image(both, root)
    K, V = em.export(both, root)
    assert np.array_equal(K, info["keys"]) and np.array_equal(V, info["vals"])
    sk = np.concatenate([np.asarray(soil[kind], dtype=U64) for kind in ib.SOIL_KINDS])
    assert sk.size >= len(ib.SOIL_KINDS)
    check_order(t, K, V, extra=sk, seed=5, what=which)
    k, v, f = t.select_batch(dev(np.arange(K.size + 1, dtype=U64)))
    t.synchronize()
    assert f.cpu().numpy()[:K.size].all() and not f.cpu().numpy()[K.size]
    assert not (host(v)[:K.size] == (host(k)[:K.size] ^ U64(ib.SOIL_XOR))).any()
    assert np.array_equal(host(k)[:K.size], K) and np.array_equal(host(v)[:K.size], V)
    t.close()


# ---- 5. batch tails ------------------------------------------------------------------

@pytest.fixture(scope="module")
def loaded(lib_ok):
    keys = bm.shape_keys(5000, "spread")
    vals = bm.shape_vals(keys)
    t = tree()
    t.bulk_load(dev(keys), dev(vals))
    yield t, keys, vals
    t.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 4097])
def test_batch_tails(loaded, n):
    """four queries per wave and sixteen per block: the last wave's and the
    last block's idle groups write nothing; the word past each output stays"""
    t, K, V = loaded
    rng = np.random.default_rng(n)
    q = K[rng.integers(0, K.size, n)] + rng.integers(0, 2, n).astype(U64)
    out = sentinels(n + 1)
    t.rank_batch(dev(q), out=out)
    assert np.array_equal(host(out)[:n], np.searchsorted(K, q, "left").astype(U64))
    assert host(out)[n] == U64(SENT)
    hi = q + rng.integers(0, 1 << 58, n).astype(U64)
    out = sentinels(n + 1)
    t.count_batch(dev(q), dev(hi), out=out)
    assert np.array_equal(host(out)[:n], want_counts(K, q, hi)) and host(out)[n] == U64(SENT)
    r = rng.integers(0, K.size + 3, n).astype(U64)
    ko, vo, fo = sentinels(n + 1), sentinels(n + 1), sentinels(n + 1, torch.uint8)
    t.select_batch(dev(r), keys=ko, vals=vo, found=fo)
    inside = r < U64(K.size)
    at = np.minimum(r, U64(K.size - 1)).astype(np.int64)
    assert np.array_equal(host(ko)[:n], np.where(inside, K[at], U64(KEY_MAX)))
    assert np.array_equal(host(vo)[:n], np.where(inside, V[at], U64(0)))
    assert np.array_equal(fo.cpu().numpy()[:n], inside.astype(np.uint8))
    assert host(ko)[n] == U64(SENT) and host(vo)[n] == U64(SENT) and fo.cpu().numpy()[n] == 0x5A
    # each output alone
    for which in range(3):
        ko, vo, fo = sentinels(n + 1), sentinels(n + 1), sentinels(n + 1, torch.uint8)
        args = [ko if which == 0 else None, vo if which == 1 else None, fo if which == 2 else None]
        rc = shm.lib().shm_select_batch(t.h, shm._ptr(dev(r)), n, *[shm._ptr(a) for a in args],
                                        None, None)
        assert rc == shm.SHM_OK
        t.synchronize()
        assert (host(ko)[:n] != U64(SENT)).all() == (which == 0)
        assert (host(vo)[:n] != U64(SENT)).all() == (which == 1)
        assert (fo.cpu().numpy()[:n] != 0x5A).all() == (which == 2)
    assert t.last_error()["bits"] == 0


def test_an_empty_batch_builds_nothing(lib_ok):
    t = tree()
    k = dev(np.arange(1, 1001, dtype=U64))
    t.insert_batch(k, k)
    none = dev(np.zeros(0, dtype=U64))
    L = shm.lib()
    assert L.shm_rank_batch(t.h, None, 0, None, None, None) == shm.SHM_OK
    assert L.shm_count_batch(t.h, None, None, 0, None, None, None) == shm.SHM_OK
    assert L.shm_select_batch(t.h, None, 0, None, None, None, None, None) == shm.SHM_OK
    assert t.rank_batch(none).numel() == 0 and t.count_batch(none, none).numel() == 0
    assert t.select_batch(none)[0].numel() == 0
    assert builds(t) == 0 and t.order_stats()["units"] == 0
    # all three outputs null with n > 0
    assert L.shm_select_batch(t.h, shm._ptr(k), 4, None, None, None, None, None) == shm.SHM_EINVAL
    assert builds(t) == 0
    t.close()


# ---- 6. validity ---------------------------------------------------------------------

def grow(seed, phases=3):
    """Random insert, overwrite and delete chunks from an empty tree, so leaves
    split and slots hold holes; the oracle holds the same tree."""
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
    return t, orc


def fresh(rng, n):
    k = rng.integers(1, KEY_MAX - 1, n, dtype=np.uint64)
    return k, k ^ U64(0x77)


def three_calls(t, K):
    """one small call of each kind"""
    q = dev(K[:8])
    t.rank_batch(q)
    t.count_batch(q, q)
    t.select_batch(dev(np.arange(8, dtype=U64)))


WRITERS = ["insert_batch", "insert_batch_async", "del_batch", "mixed_batch", "insert_apply",
           "bulk_load", "compact", "load_image"]


@pytest.fixture(scope="module")
def grown(lib_ok):
    t, orc = grow(11)
    orc.close()
    yield t
    t.close()


def test_a_valid_index_is_not_rebuilt(grown):
    """the first call builds; the next calls of any kind, and the readers
    between them, leave the index alone"""
    t = grown
    K, V, _ = model_of(t)
    k0 = dev(K[:64])
    t.insert_batch(k0, dev(V[:64]))  # whatever an earlier test left: stale now
    b = builds(t)
    t.rank_batch(k0)
    assert builds(t) == b + 1
    for _ in range(2):
        three_calls(t, K)
    assert builds(t) == b + 1
    v = torch.empty_like(k0)
    t.search_batch(k0, v, torch.empty(64, dtype=torch.uint8, device="cuda"))
    t.export(int(K[10]), int(K[500]))
    assert t.count() == K.size
    t.scan_batch(k0, 10).result()
    t.rscan_batch(k0, 10).result()
    t.set_key_range(0, 64)
    t.synchronize()
    three_calls(t, K)
    assert builds(t) == b + 1
    check_order(t, K, V, seed=6, what="valid")
    assert builds(t) == b + 1


@pytest.mark.parametrize("writer", WRITERS)
def test_every_writer_makes_the_index_stale(grown, writer):
    """After each writer the next call rebuilds exactly once, and its results
    equal the model on a fresh dump_image().  Each case fails when the bump of
    shm_tree::ord_gen that it guards is removed: insert_batch,
    insert_batch_async (no synchronise in between), del_batch, mixed_batch and
    insert_apply guard the one in insert_finish (tree_insert.cpp), which every
    insert chunk passes; bulk_load and compact the one in bulk_load_locked
    (tree_image.cpp); load_image the one in shm_load_image (tree_image.cpp)."""
    t = grown
    rng = np.random.default_rng(WRITERS.index(writer))
    K, V, _ = model_of(t)
    three_calls(t, K)  # valid from here
    b = builds(t)
    nk, nv = fresh(rng, 3000)
    kd, vd = dev(nk), dev(nv)
    torch.cuda.synchronize()
    if writer == "insert_batch":
        t.insert_batch(kd, vd)
    elif writer == "insert_batch_async":
        t.insert_batch_async(kd, vd, stream=torch.cuda.Stream())
    elif writer == "del_batch":
        t.del_batch(dev(K[::3][:3000]))
    elif writer == "mixed_batch":
        g = dev(K[:16])
        t.mixed_batch(g, torch.empty_like(g), torch.empty(16, dtype=torch.uint8, device="cuda"),
                      kd, vd)
    elif writer == "insert_apply":
        tk = t.insert_order(kd, vd)
        with pytest.raises(shm.ShermanError) as e:
            t.rank_batch(kd)
        assert e.value.rc == shm.SHM_EINVAL
        with pytest.raises(shm.ShermanError) as e:
            t.count_batch(kd, kd)
        assert e.value.rc == shm.SHM_EINVAL
        with pytest.raises(shm.ShermanError) as e:
            t.select_batch(kd)
        assert e.value.rc == shm.SHM_EINVAL
        assert builds(t) == b  # the ordered chunk changed nothing yet
        t.insert_apply(tk)
    elif writer == "bulk_load":
        keep = np.unique(np.concatenate([K[::2], nk]))
        t.bulk_load(dev(keep), dev(keep ^ U64(0x99)), 20, 30)
    elif writer == "compact":
        t.compact(53, 60)
    elif writer == "load_image":
        img, root, _ = entry_states()
        t.load_image(img, root)
    # the call itself: no synchronise since the writer
    got = host(t.rank_batch(dev(np.array([KEY_MAX], dtype=U64))))
    assert builds(t) == b + 1, writer
    K2, V2, _ = model_of(t)
    assert int(got[0]) == K2.size, writer
    if writer == "compact":
        assert np.array_equal(K2, K) and np.array_equal(V2, V)
    else:
        assert not np.array_equal(K2, K), "the writer wrote nothing"
    if writer in ("insert_batch", "insert_batch_async", "mixed_batch", "insert_apply"):
        assert np.isin(nk, K2).all()
    check_order(t, K2, V2, extra=nk[:100], seed=7, what=writer)
    assert builds(t) == b + 1, writer
    t.check()


def test_the_calls_change_nothing(lib_ok):
    """dump_image(), stats(), dir_stats() and vt_stats() are the same before
    and after a batch of each call, the rebuilding one included"""
    t, orc = grow(12, phases=2)
    orc.close()
    K, V, _ = model_of(t)
    for _ in range(6):  # a read phase: the directory and the table are built
        k = dev(K[:4096])
        t.search_batch(k, torch.empty_like(k), torch.empty(4096, dtype=torch.uint8, device="cuda"))
    t.synchronize()
    assert t.dir_stats()["builds"] >= 1
    before = (t.dump_image(), t.stats(), t.dir_stats(), t.vt_stats())
    b = builds(t)
    check_order(t, K, V, seed=8, what="read-only")
    assert builds(t) == b + 1
    after = (t.dump_image(), t.stats(), t.dir_stats(), t.vt_stats())
    assert before[0][1] == after[0][1] and np.array_equal(before[0][0], after[0][0])
    assert before[1:] == after[1:], (before[1:], after[1:])
    t.close()


# ---- 7. against the oracle -----------------------------------------------------------

def test_grown_tree_against_the_oracle(lib_ok):
    t, orc = grow(13)
    ok, ov = orc.dump()
    o = np.argsort(ok, kind="stable")
    ok, ov = ok[o], ov[o]
    orc.close()
    assert 25000 < ok.size < 60000 and t.stats()["root_level"] >= 2
    got = host(t.rank_batch(dev(ok)))
    assert np.array_equal(got, np.arange(ok.size, dtype=U64))
    k, v, f = t.select_batch(dev(np.arange(ok.size, dtype=U64)))
    assert f.cpu().numpy().all()
    assert np.array_equal(host(k), ok) and np.array_equal(host(v), ov)
    K, V, _ = model_of(t)
    assert np.array_equal(K, ok) and np.array_equal(V, ov)
    assert t.last_error()["bits"] == 0
    t.close()


# ---- 8. quantiles --------------------------------------------------------------------

def test_quantile_keys(loaded):
    t, K, _ = loaded
    N = K.size
    for parts in (2, 3, 8, 16):
        q = host(t.quantile_keys(parts))
        assert np.array_equal(q, K[[p * N // parts for p in range(1, parts)]]), parts
    cuts = shm.rebalance_plan([N], 0)["cut"]
    assert cuts == [0, N]
    assert t.quantile_keys(1).numel() == 0


def test_quantile_keys_of_a_small_tree(lib_ok):
    t = tree()
    k = np.array([5, 9, 1 << 63, KEY_MAX - 1, 77], dtype=U64)
    t.insert_batch(dev(k), dev(k))
    K = np.sort(k)
    for parts in (2, 3, 5):
        q = host(t.quantile_keys(parts))
        assert np.array_equal(q, K[[p * 5 // parts for p in range(1, parts)]]), parts
    for parts in (6, 8, 16):  # fewer pairs than parts
        assert t.quantile_keys(parts).numel() == 0
    t.close()


# ---- 9. size -------------------------------------------------------------------------

def test_a_million_keys(lib_ok):
    """2^20 hashed keys grown by inserts; 2^16 random keys, ranks and ranges"""
    N, Q = 1 << 20, 1 << 16
    t = shm.Tree(arena_bytes=128 << 20, max_batch=N // 4)
    kd = torch.empty(N, dtype=torch.int64, device="cuda")
    t.gen_keys(1, N, kd)
    for at in range(0, N, N // 4):
        part = kd[at:at + N // 4]
        t.insert_batch(part, part ^ 0x2222)
    K, V, _ = model_of(t)
    assert K.size == N and t.stats()["root_level"] >= 2
    rng = np.random.default_rng(9)
    q = np.concatenate([K[rng.integers(0, N, Q // 2)],
                        rng.integers(0, KEY_MAX, Q // 2, dtype=np.uint64)])
    got = host(t.rank_batch(dev(q)))
    assert np.array_equal(got, np.searchsorted(K, q, "left").astype(U64))
    r = rng.integers(0, N + N // 64, Q).astype(U64)
    k, v, f = t.select_batch(dev(r))
    inside = r < U64(N)
    at = np.minimum(r, U64(N - 1)).astype(np.int64)
    assert np.array_equal(f.cpu().numpy(), inside.astype(np.uint8))
    assert np.array_equal(host(k), np.where(inside, K[at], U64(KEY_MAX)))
    assert np.array_equal(host(v), np.where(inside, V[at], U64(0)))
    hi = q + (rng.integers(0, KEY_MAX, Q, dtype=np.uint64) >> rng.integers(1, 60, Q).astype(U64))
    hi[hi < q] = U64(KEY_MAX)
    got = host(t.count_batch(dev(q), dev(hi)))
    assert np.array_equal(got, want_counts(K, q, hi))
    st = t.order_stats()
    assert st["builds"] == 1 and st["pairs"] == N and 0 < st["units"] <= t.check()["leaves"]
    assert t.last_error()["bits"] == 0
    t.close()
