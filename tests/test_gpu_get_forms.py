"""The two forms of k_get_sum's front (get_sum.hip) behind a bucket table: the
cooperative probe (SHM_GET_COOP: eight lanes load one bucket line, the owner
lane gets vt_probe's answer back) and the packing of the gets the table does
not answer into the block's lowest waves (SHM_GET_PACK).  Every batch runs on
one tree in the four combinations of the two switches (Tree.get_forms: the
forms of a tree's later launches, as the variables set them at its creation),
and each must give the oracle's values and found flags and the seven index
statistics of the 0,0 form on the same batch and the same tree (two trees of
the same keys differ in their leaves' slot order, and so in the entries a
walk reads).

Shapes: 2^16 hashed keys plus 64 runs of 12 adjacent keys (dead buckets where
the test wants them), a 128 MB arena, chunks of at most 2^16 ops, five
searches to reach the read phase.  The probes are classified by the host
models (valtab_model.py, get_paths.py) on the table's and the directory's
dumps, so each case checks that its batch is what its name says.
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

import get_paths as gp  # noqa: E402
import valtab_model as vm  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, U64  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402
from sherman_amd.shard import shard_range  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_MAX = U64(shm.KEY_MAX)
N0 = 1 << 16
MB = 1 << 16
ARENA = 128 << 20
TPB = 256  # kernels.h kGetSumTPB
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (SHM_GET_COOP, SHM_GET_PACK)


def hashed_keys(first, n):
    t = shm.Tree(arena_bytes=ARENA, max_batch=MB)
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    t.gen_keys(first, n, k)
    torch.cuda.synchronize()
    out = k.cpu().numpy().view(U64).copy()
    t.close()
    return out


def search(t, keys, found=True):
    """(values, found flags or None, the batch's own index statistics)"""
    k = dev(keys)
    v = torch.empty_like(k)
    f = torch.empty(k.numel(), dtype=torch.uint8, device="cuda") if found else None
    t.profile(False, index_stats=True)
    t.index_stats()  # (reset)
    try:
        t.search_batch(k, v, f)
        t.synchronize()
        st = t.index_stats()
    finally:
        t.profile(False)
    return v.cpu().numpy().view(U64), (f.cpu().numpy() if found else None), st


class Rig:
    """A tree in its read phase and its oracle."""

    def __init__(self, keys, table=True, **kw):
        self.kw = kw
        keys = np.unique(np.asarray(keys, dtype=U64))
        vals = (keys * U64(2654435761)) | U64(1)  # never 0
        self.orc = OracleTree(ARENA)
        self.orc.apply_batch(keys, vals)
        self.stored = keys
        self.t = t = shm.Tree(arena_bytes=ARENA, max_batch=MB, **kw)
        t.dir_config(maint="always")
        for c in range(0, keys.size, MB):
            t.insert_batch(dev(keys[c:c + MB]), dev(vals[c:c + MB]))
        for _ in range(5):
            search(t, keys[:4096])
        assert t.dir_stats()["form"] == "pairs", t.dir_stats()
        self.page_check = bool(kw.get("page_check", False))
        if table:
            self.remodel()

    def remodel(self):
        """the table's geometry and the stored keys' buckets, from the dump"""
        self.buckets, info = self.t.vt_dump()
        assert self.buckets.shape[0] and info["trusted"], (self.buckets.shape, info)
        self.lo, self.shift, self.n = info["lo"], info["shift"], self.buckets.shape[0]
        self.dead = vm.dead(self.buckets)
        self.stored, _ = self.orc.dump()
        self.stored = np.sort(self.stored)
        self.home = vm.bucket_of(self.stored, self.lo, self.shift)
        self.count = vm.counts(self.stored, self.lo, self.shift, self.n)

    def classes(self, keys):
        return gp.classify(keys, *gp.dumps(self.t, self.page_check))

    def in_table(self, home):
        return (home >= 0) & (home < self.n)

    def stored_in(self, dead):
        """stored keys whose bucket is dead (True) / live (False)"""
        ok = self.in_table(self.home)
        ok[ok] &= self.dead[self.home[ok]] == dead
        return self.stored[ok]

    def fresh_in(self, buckets, rng):
        """one never-stored key inside each given bucket"""
        low = rng.integers(1, 1 << self.shift, buckets.size).astype(U64)
        k = U64(self.lo) + (buckets.astype(U64) << U64(self.shift)) + low
        k = np.unique(k[~np.isin(k, self.stored)])
        return k[k != KEY_MAX]

    def falls(self, keys):
        """the gets the table does not answer (and that are gets at all)"""
        return (self.classes(keys) != gp.TABLE) & (np.asarray(keys, dtype=U64) != KEY_MAX)

    def check(self, keys, label, found=True):
        """One batch in the four forms: the oracle's answers, and the 0,0
        form's seven statistics.  Returns those statistics."""
        keys = np.ascontiguousarray(keys, dtype=U64)
        ov, of = self.orc.search_batch(keys)
        ref = None
        for c in COMBOS:
            self.t.get_forms(*c)
            gv, gf, st = search(self.t, keys, found)
            if found:
                gp.assert_equal(keys, ov, of, gv, gf)
            else:
                gp.assert_equal(keys, ov, of, gv, of)
            assert st["gets"] == int((keys != KEY_MAX).sum()), (label, c, st)
            if ref is None:
                ref = st
                print(f"{label}: n={keys.size} fall-through={int(self.falls(keys).sum())} {st}")
            assert st == ref, (label, c, st, ref)
            assert self.t.last_error()["bits"] == 0, (label, c)
        self.t.get_forms(1, 1)
        return ref

    def close(self):
        self.t.close()
        self.orc.close()


def clustered(rng, lo=0, end=1 << 64, n_runs=64, run=12):
    """runs of adjacent keys: more than 8 keys of one bucket, whatever its width"""
    anchors = rng.integers(lo + (1 << 40), end - (1 << 40), n_runs, dtype=np.uint64)
    return np.unique((anchors[:, None] + np.arange(1, run + 1, dtype=U64)[None, :]).ravel())


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    rng = np.random.default_rng(101)
    cl = clustered(rng)
    r = Rig(np.concatenate([hashed_keys(1, N0), cl, np.zeros(1, dtype=U64)]))
    r.cl = cl
    # the clustered runs did make dead buckets
    assert r.dead[r.home[np.isin(r.stored, cl)]].mean() > 0.9
    yield r
    r.close()


@pytest.fixture(scope="module")
def shard_rig():
    """a tree made with shard 5 of 8's range, holding keys below, inside and
    above it, the range's first and last key and key 0"""
    assert torch.cuda.is_available(), "GPU test without a GPU"
    lo, bits = shard_range(5, 8)
    end = lo + (1 << bits)
    h = hashed_keys(1, N0)
    rng = np.random.default_rng(102)
    inside = U64(lo) + (h[:N0 - 2048] >> U64(64 - bits))
    cl = clustered(rng, lo, end)
    below = h[N0 - 2048:N0 - 1024] % U64(lo)
    above = U64(end) + h[N0 - 1024:] % U64((1 << 64) - 1 - end)
    r = Rig(np.concatenate([inside, cl, below, above, np.array([0, lo, end - 1], dtype=U64)]),
            key_lo=lo, key_bits=bits)
    assert r.lo == lo and lo + (r.n << r.shift) == end, (r.lo, r.n, r.shift)
    r.range, r.below, r.above = (lo, end), np.unique(below), np.unique(above)
    yield r
    r.close()


def table_pool(r, rng, n):
    """n probes the table answers: stored keys and absent keys of live buckets"""
    live = r.stored_in(False)
    absent = r.fresh_in(rng.permutation(np.nonzero(~r.dead & (r.count > 0))[0])[:n // 4 + 1], rng)
    k = np.concatenate([live[rng.integers(0, live.size, n)], absent])
    k = rng.permutation(k)[:n]
    assert (r.classes(k) == gp.TABLE).all()
    return k


def fall_pool(r, rng, n):
    """n distinct probes of dead buckets: stored keys, then absent ones"""
    dead_b = np.nonzero(r.dead)[0]
    k = np.concatenate([rng.permutation(r.stored_in(True)), r.fresh_in(dead_b, rng)])[:n]
    assert k.size == n and r.falls(k).all(), (k.size, n)
    return k


def placed(r, rng, size, positions):
    """a batch of `size` table-answered probes with fall-through gets at
    exactly `positions`"""
    positions = np.asarray(positions, dtype=np.int64)
    k = table_pool(r, rng, size)
    k[positions] = rng.permutation(fall_pool(r, rng, positions.size))
    f = r.falls(k)
    assert np.array_equal(np.nonzero(f)[0], np.sort(positions))
    return k


@pytest.mark.parametrize("size", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_with_idle_lanes_and_waves(rig, size):
    """A mixed batch of every size at which the last block has idle lanes or
    idle waves: stored and absent keys of live buckets, and one probe in
    eight of a dead bucket (at size 1: one of each)."""
    rng = np.random.default_rng(200 + size)
    k = table_pool(rig, rng, size)
    fp = fall_pool(rig, rng, max(1, size // 8))
    at = rng.permutation(size)[:fp.size]
    k[at] = fp
    rig.check(k, f"size {size}")
    if size == 1:
        rig.check(table_pool(rig, rng, 1), "size 1, table")


def test_no_fall_through_get(rig):
    """Every get is the table's: no wave goes on past the barrier, and no
    leaf entry is read."""
    rng = np.random.default_rng(210)
    for size in (256, 1000):
        st = rig.check(table_pool(rig, rng, size), f"table only {size}")
        assert st["entry_reads"] == 0 and st["dir_fp_hits"] == st["hits"], st


def test_only_fall_through_gets(rig):
    """256 and more stored keys of dead buckets: all four waves of a block go
    on, each full; then with a last block of one wave and one lane."""
    rng = np.random.default_rng(211)
    dead_stored = rig.stored_in(True)
    assert dead_stored.size >= 2 * TPB + 65, dead_stored.size
    for size in (TPB, TPB + 1, 2 * TPB + 65):
        k = rng.permutation(dead_stored)[:size]
        assert rig.falls(k).all()
        st = rig.check(k, f"dead only {size}")
        assert st["hits"] == size, st


@pytest.mark.parametrize("n_fall", [1, 63, 64, 65, 128, 129])
def test_fall_through_count_at_the_wave_edges(rig, n_fall):
    """The middle block of three holds exactly n_fall fall-through gets,
    spread over its four waves (and, again, all at its front and all at its
    back); its neighbours hold none and three: 64 fill one wave, 65 need a
    second."""
    rng = np.random.default_rng(220 + n_fall)
    for how in ("spread", "front", "back"):
        if how == "spread":
            pos = TPB + np.sort(rng.permutation(TPB)[:n_fall])
        elif how == "front":
            pos = TPB + np.arange(n_fall)
        else:
            pos = 2 * TPB - 1 - np.arange(n_fall)
        pos = np.concatenate([pos, [2 * TPB + 5, 2 * TPB + 70, 3 * TPB - 1]])
        rig.check(placed(rig, rng, 3 * TPB, pos), f"{n_fall} fall-through, {how}")


@pytest.mark.parametrize("n_fall", [1, 10, 64])
def test_fall_through_in_the_last_wave_only(rig, n_fall):
    """All of a block's fall-through gets sit in its last wave, so wave 0
    takes over gets that only wave 3 held; also in a last block whose last
    wave is partly idle."""
    rng = np.random.default_rng(230 + n_fall)
    pos = 3 * 64 + np.sort(rng.permutation(64)[:n_fall])
    rig.check(placed(rig, rng, TPB, pos), f"last wave, {n_fall}")
    pos2 = np.concatenate([pos[pos < 3 * 64 + 40], TPB + pos[pos < 3 * 64 + 40]])
    if pos2.size:
        rig.check(placed(rig, rng, 2 * TPB - 24, pos2), f"last wave of a short block, {n_fall}")


def test_dead_bucket_keys_by_answering_path(rig):
    """Dead-bucket keys that the directory's value form answers, that the
    pairs answer from a leaf, and that are absent, each class alone and all
    mixed with table probes."""
    rng = np.random.default_rng(240)
    ds = rig.stored_in(True)
    cls = rig.classes(ds)
    by_value, by_pairs = ds[cls == gp.VALUE], ds[cls == gp.LEAF]
    absent = rig.fresh_in(np.nonzero(rig.dead)[0], rng)
    print(f"dead-bucket stored keys: value form {by_value.size}, pairs {by_pairs.size}; "
          f"absent {absent.size}")
    assert by_value.size and by_pairs.size and absent.size
    st = rig.check(by_value, "dead, value form")
    assert st["hits"] == by_value.size and st["entry_reads"] == 0, st
    st = rig.check(by_pairs, "dead, pairs")
    assert st["hits"] == by_pairs.size and st["entry_reads"] >= by_pairs.size, st
    st = rig.check(absent, "dead, absent")
    assert st["hits"] == 0, st
    mix = rng.permutation(np.concatenate([by_value, by_pairs[:500], absent[:200],
                                          table_pool(rig, rng, 1500)]))
    rig.check(mix, "dead, mixed")


def test_absent_keys_inside_live_buckets(rig):
    """Never-stored keys of live buckets holding 0, 1..7 and 8 keys: absent
    from the table alone."""
    rng = np.random.default_rng(241)
    live = ~rig.dead
    for name, sel in (("empty", live & (rig.count == 0)), ("part", live & (rig.count > 0)),
                      ("full", live & (rig.count == vm.SLOTS))):
        b = rng.permutation(np.nonzero(sel)[0])[:700]
        assert b.size >= 16, (name, b.size)
        k = rig.fresh_in(b, rng)
        assert (rig.classes(k) == gp.TABLE).all()
        st = rig.check(k, f"absent in {name} buckets")
        assert st["hits"] == 0 and st["entry_reads"] == 0, st


def test_one_key_64_times_and_one_bucket_8_times(rig):
    """One wave of 64 copies of one key (a table key, a dead-bucket key, key
    0); and the eight keys of one full live bucket in one wave: in eight
    adjacent lanes (one round, eight lane groups on one line), in lanes 8
    apart (one lane group, eight rounds), and the same for eight keys of a
    dead bucket."""
    rng = np.random.default_rng(242)
    one_live = rig.stored_in(False)[7]
    one_dead = rig.stored_in(True)[7]
    for name, key in (("table", one_live), ("dead", one_dead), ("zero", U64(0))):
        st = rig.check(np.full(64, key, dtype=U64), f"64 x one {name} key")
        assert st["hits"] == 64, st
        k = table_pool(rig, rng, TPB)
        k[64:128] = key
        rig.check(k, f"64 x one {name} key in wave 1")
    full = np.nonzero(~rig.dead & (rig.count == vm.SLOTS))[0]
    deadb = np.nonzero(rig.dead & (rig.count >= vm.SLOTS))[0]
    assert full.size and deadb.size
    for name, b in (("live", full[0]), ("dead", deadb[0])):
        eight = rig.stored[rig.home == b][:8]
        assert eight.size == 8
        for how, lanes in (("adjacent", 16 + np.arange(8)), ("strided", 3 + 8 * np.arange(8))):
            k = table_pool(rig, rng, 64)
            k[lanes] = eight
            st = rig.check(k, f"8 keys of one {name} bucket, {how}")
            assert st["hits"] >= 8, st
        st = rig.check(np.tile(eight, 8), f"8 keys of one {name} bucket x 8")
        assert st["hits"] == 64, st


def specials(r):
    lo, end = getattr(r, "range", (0, 1 << 64))
    k = [0, 1, int(KEY_MAX), int(KEY_MAX) - 1, lo, lo + 1, end - 1, end - 2]
    if lo:
        k += [lo - 1, end % (1 << 64), end + 1, int(r.below[0]), int(r.below[-1]),
              int(r.above[0]), int(r.above[-1])]
    return np.array(k, dtype=U64)


@pytest.mark.parametrize("which", ["whole", "shard"])
def test_key_zero_key_max_and_the_range_ends(rig, shard_rig, which):
    """Key 0, KEY_MAX, the first and last keys of the table's range and,
    under a shard range, stored and absent keys below key_lo and above the
    range: each alone, all together, and mixed into a full batch at the wave
    and block edges."""
    r = rig if which == "whole" else shard_rig
    rng = np.random.default_rng(250)
    sp = specials(r)
    cls = r.classes(sp)
    assert cls[0] != gp.TABLE and cls[2] != gp.TABLE
    if which == "shard":
        home = vm.bucket_of(sp, r.lo, r.shift)
        assert home[4] == 0 and home[6] == r.n - 1 and home[8] == -1 and home[9] >= r.n
        assert (cls[8:] != gp.TABLE).all() and (cls[4:8] == gp.TABLE).any()
        assert np.isin(r.below, r.stored).all()
    for k in sp:
        r.check(np.array([k], dtype=U64), f"{which}: key {int(k):#x} alone")
    r.check(sp, f"{which}: specials together")
    full = table_pool(r, rng, 2 * TPB + 100)
    at = np.array([0, 63, 64, 127, 128, 191, 192, 255, 256, 300, 319, 2 * TPB + 99,
                   2 * TPB + 64, 2 * TPB + 63, 511])[:sp.size]
    full[at] = sp
    r.check(full, f"{which}: specials in a full batch")
    if which == "shard":
        out = rng.permutation(np.concatenate([r.below, r.above]))[:700]
        st = r.check(np.concatenate([out, full]), "shard: a block of keys outside the range")
        assert st["hits"] >= out.size, st


def test_after_a_kept_chunk_and_after_the_trust_ends():
    """Chunks the table keeps (updates, deletes, re-inserts and new keys in
    probed buckets, one overflowing a bucket), then the probes of the touched
    buckets; then a chunk without upkeep, after which no launch has a table
    (one instantiation whatever the switches) and the same probes still equal
    the oracle."""
    rng = np.random.default_rng(260)
    r = Rig(np.concatenate([hashed_keys(1, N0), clustered(rng)]))
    live = r.stored_in(False)
    pick = rng.permutation(live.size)
    upd, dele = live[pick[:2000]], live[pick[2000:4000]]
    new = r.fresh_in(rng.permutation(np.nonzero(~r.dead)[0])[:2000], rng)
    touched_b = np.unique(vm.bucket_of(np.concatenate([upd, dele, new]), r.lo, r.shift))
    probe = np.unique(np.concatenate([r.stored[np.isin(r.home, touched_b)], new, dele + U64(1),
                                      r.stored_in(True)[:1000]]))
    probe = rng.permutation(probe[probe != KEY_MAX])
    chunks = [(np.concatenate([upd, dele]),
               np.concatenate([upd ^ U64(0x5A5A5A) | U64(1), np.zeros(dele.size, dtype=U64)])),
              (np.concatenate([dele[:1000], new]),
               np.concatenate([dele[:1000] ^ U64(0xC3C3C3) | U64(1), new | U64(1)]))]
    for n, (k, v) in enumerate(chunks):
        r.orc.apply_batch(k, v)
        r.t.insert_batch(dev(k), dev(v))
        assert r.t.vt_stats()["trusted"], (n, r.t.vt_stats())
        r.remodel()
        bad = vm.check(r.buckets, r.lo, r.shift, *r.orc.dump())
        assert bad == [], bad[:8]
        st = r.check(probe, f"after kept chunk {n}")
        assert st["dir_fp_hits"] > 0, st
    k, v = live[pick[4000:6000]], live[pick[4000:6000]] ^ U64(0x77) | U64(1)
    r.orc.apply_batch(k, v)
    r.t.dir_config(maint=False)
    r.t.insert_batch(dev(k), dev(v))
    assert not r.t.vt_stats()["trusted"]
    r.check(np.concatenate([probe, k]), "after the trust ended")
    r.close()


def test_null_found_and_page_check(rig):
    """found=None reaches the kernel as a null out_found: values alone, the
    same statistics.  A tree made with page_check=True never probes the
    table, whatever the switches: every hit reads a leaf entry."""
    rng = np.random.default_rng(270)
    k = table_pool(rig, rng, 3 * TPB + 17)
    fp = fall_pool(rig, rng, 150)
    k[rng.permutation(k.size)[:fp.size]] = fp
    k[5], k[700] = KEY_MAX, U64(0)
    st = rig.check(k, "found=None", found=False)
    assert st == rig.check(k, "found given")
    pc = Rig(rig.stored, table=False, page_check=True)
    assert (pc.classes(k) == gp.LEAF).all()
    st = pc.check(k, "page_check=True")
    assert st["entry_reads"] >= st["hits"] > 0, st
    pc.close()


def test_the_environment_sets_a_new_tree_s_forms(rig):
    """SHM_GET_COOP and SHM_GET_PACK are read when a tree is created: trees
    made under each combination answer a mixed batch as the oracle does."""
    rng = np.random.default_rng(280)
    k = table_pool(rig, rng, 2 * TPB + 31)
    fp = fall_pool(rig, rng, 90)
    k[rng.permutation(k.size)[:fp.size]] = fp
    ov, of = rig.orc.search_batch(k)
    vals = (rig.stored * U64(2654435761)) | U64(1)
    for coop, pack in COMBOS:
        def make():
            t = shm.Tree(arena_bytes=ARENA, max_batch=MB)
            t.dir_config(maint="always")
            for c in range(0, rig.stored.size, MB):
                t.insert_batch(dev(rig.stored[c:c + MB]), dev(vals[c:c + MB]))
            for _ in range(5):
                search(t, rig.stored[:4096])
            return t
        t = gp.with_env("SHM_GET_COOP", str(coop),
                        lambda: gp.with_env("SHM_GET_PACK", str(pack), make))
        assert t.vt_stats()["trusted"]
        gv, gf, _ = search(t, k)
        gp.assert_equal(k, ov, of, gv, gf)
        assert t.last_error()["bits"] == 0
        t.close()
