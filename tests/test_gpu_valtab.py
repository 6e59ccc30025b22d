"""The key-value bucket table (csrc/valtab.h): a read phase's get reads one
128 B bucket of 8 (key, value) slots first and ends there unless the bucket
overflowed (dead).  Builds, the chunks' upkeep, the end of trust, the
switches and the drop rule are checked against the CPU oracle and by the host
model of the bucket format (tests/valtab_model.py) on raw dumps.

Shapes follow test_gpu_dir_vals.py: 2^18 hashed keys, a 512 MB arena, chunks
of at most 2^18 ops, five searches to reach the read phase: 2^17 directory
entries, so 2^16 buckets of four keys on average.
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

import valtab_model as vm  # noqa: E402
from get_paths import with_env, without_table  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import (assert_same, dev, gen_keys, gpu_search,  # noqa: E402
                         gpu_search_stats, host, lib_ok, U64)
from oracle.pyoracle import OracleTree  # noqa: E402

pytestmark = pytest.mark.gpu

N0 = 1 << 18
ARENA = 512 << 20


def loaded(maint="always", max_batch=1 << 18, keys=None, mem_limit=0, **kw):
    """A tree of N0 hashed keys (or `keys`) in its read phase (five
    searches), and its oracle."""
    t = shm.Tree(arena_bytes=ARENA, max_batch=max_batch, **kw)
    t.dir_config(maint=maint, mem_limit=mem_limit)
    orc = OracleTree(ARENA)
    base = gen_keys(t, 1, N0) if keys is None else keys
    bv = np.arange(1, base.size + 1, dtype=U64) * U64(2)
    for c in range(0, base.size, max_batch):
        t.insert_batch(dev(base[c:c + max_batch]), dev(bv[c:c + max_batch]))
    orc.apply_batch(base, bv)
    for _ in range(5):
        gpu_search(t, base[:4096])
    d = t.dir_stats()
    assert d["form"] == "pairs", d
    return t, orc, base


class Buckets:
    """The table's buckets of a key set, on the host."""

    def __init__(self, t, keys):
        _, info = t.vt_dump()
        st = t.vt_stats()
        assert st["buckets"], st
        self.n = st["buckets"]
        self.lo, self.shift = info["lo"], info["shift"]
        self.keys = np.sort(keys)
        self.home = vm.bucket_of(self.keys, self.lo, self.shift)
        self.count = vm.counts(keys, self.lo, self.shift, self.n)

    def of(self, k):
        return vm.bucket_of(k, self.lo, self.shift)

    def members(self, buckets):
        return self.keys[np.isin(self.home, buckets)]

    def fresh_in(self, buckets, rng, stored):
        """one key, not stored, inside each given bucket"""
        low = rng.integers(1, 1 << self.shift, buckets.size).astype(U64)
        k = U64(self.lo) + (buckets.astype(U64) << U64(self.shift)) + low
        k = np.unique(k[~np.isin(k, stored)])
        return k[k != U64(shm.KEY_MAX)]


def model_clean(t, orc):
    bad, info = vm.check_tree(t, *orc.dump())
    assert bad == [], bad[:8]
    return info


def test_build_answers_most_gets_from_one_bucket(lib_ok):
    """The build: exactly the buckets of more than 8 stored keys are dead,
    every other bucket holds its keys (host model), a stored batch whose
    share p of probes lies in live buckets reads at most 1.05 (1 - p) leaf
    entries per get while every get is answered from the table or the
    directory entry, and never-stored keys are absent."""
    t, orc, base = loaded()
    st = t.vt_stats()
    assert st["trusted"] and st["buckets"] == 1 << 16 and st["bytes"] == 128 << 16, st
    bk = Buckets(t, base)
    over = bk.count > vm.SLOTS
    assert st["dead_buckets"] == int(over.sum()), (st, int(over.sum()))
    assert st["keys_at_build"] == N0, st
    assert st["dead_keys_at_build"] == int(bk.count[over].sum()), st
    buckets, _ = t.vt_dump()
    assert np.array_equal(vm.dead(buckets), over)
    model_clean(t, orc)
    rng = np.random.default_rng(31)
    probe = base[rng.integers(0, N0, 1 << 15)]
    p = float(np.mean(bk.count[bk.of(probe)] <= vm.SLOTS))
    assert p > 0.9, p  # uniform keys, four per bucket: 0.948
    gv, gf, s = gpu_search_stats(t, probe)
    assert_same(probe, *orc.search_batch(probe), gv, gf)
    print(f"p={p:.4f} gets={s['gets']} entry_reads={s['entry_reads']} "
          f"dir_fp_hits={s['dir_fp_hits']} bound={1.05 * (1 - p) * s['gets']:.0f}")
    assert s["dir_fp_hits"] == s["gets"], s
    assert s["entry_reads"] <= 1.05 * (1 - p) * s["gets"], (p, s)
    absent = gen_keys(t, N0 + 1, 1 << 13)
    gv, gf, s = gpu_search_stats(t, absent)
    assert_same(absent, *orc.search_batch(absent), gv, gf)
    assert not gf.any() and s["dir_fp_hits"] <= s["hits"], s
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


def test_chunks_keep_the_table_equal_to_the_tree(lib_ok):
    """Upkeep on for every chunk, one chunk each: in-place updates, deletes,
    re-inserts of the deleted keys with new values (the freed slot is reused,
    no duplicate), a mixed chunk that puts re-inserts of deleted keys, deletes
    of already deleted keys, deletes of live keys and new keys into the same
    buckets in one launch (a slot claimed by one op must never match another
    op's key), key 0 (which never uses the table), new keys into buckets
    holding 0, 3, 7 and 8 keys (the last overflows: dead), and runs of 30
    adjacent new keys into empty buckets (leaf splits; more than 8 claims of
    one empty bucket in one launch, where the marker must survive a racing
    claim of slot 0).  After each: the
    touched keys and their buckets' other keys equal the oracle, the model is
    clean, nothing was rebuilt, no error."""
    t, orc, base = loaded()
    bk = Buckets(t, base)
    rng = np.random.default_rng(32)
    builds = t.dir_stats()["builds"]
    live_keys = bk.keys[bk.count[bk.home] <= vm.SLOTS]
    pick = rng.permutation(live_keys.size)
    upd, dele = live_keys[pick[:3000]], live_keys[pick[3000:6000]]
    taken = np.unique(np.concatenate([bk.of(upd), bk.of(dele)]))
    free = np.setdiff1d(np.arange(bk.n), taken)
    by_count = {c: rng.permutation(free[bk.count[free] == c]) for c in (0, 3, 7, 8)}
    assert all(v.size >= 300 for v in by_count.values()), {c: v.size for c, v in by_count.items()}
    new_b = np.concatenate([by_count[c][:300] for c in (0, 3, 7, 8)])
    new = bk.fresh_in(new_b, rng, base)
    full = by_count[8][:300]
    empty = by_count[0][300:400]
    assert empty.size >= 50
    anchors = U64(bk.lo) + (empty.astype(U64) << U64(bk.shift)) + \
        rng.integers(1, 1 << (bk.shift - 1), empty.size).astype(U64)
    runs = np.unique((anchors[:, None] + np.arange(1, 31, dtype=U64)[None, :]).ravel())
    sample = base[rng.integers(0, N0, 1 << 13)]
    # the mixed chunk: buckets of 3 to 6 keys away from everything above; of
    # each bucket's keys the first is deleted beforehand ("delete2") and then
    # re-inserted (even buckets) or deleted again (odd buckets), the second is
    # deleted, and two new keys arrive, all in one launch
    used = np.unique(np.concatenate([taken, new_b, empty]))
    mix_b = np.setdiff1d(np.nonzero((bk.count >= 3) & (bk.count <= 6))[0], used)
    mix_b = rng.permutation(mix_b)[:4000]
    assert mix_b.size >= 2000
    first = np.searchsorted(bk.home, mix_b)  # bk.keys is sorted, so is bk.home
    k_first, k_second = bk.keys[first], bk.keys[first + 1]
    even = (np.arange(mix_b.size) % 2) == 0
    mix_new = np.concatenate([bk.fresh_in(mix_b, rng, base), bk.fresh_in(mix_b, rng, base)])
    mix_new = np.unique(mix_new)
    mix_k = np.concatenate([k_first, k_second, mix_new, np.zeros(1, dtype=U64)])
    mix_v = np.concatenate([np.where(even, k_first ^ U64(0xF00D), U64(0)),
                            np.zeros(k_second.size, dtype=U64), mix_new ^ U64(0xBEEF),
                            np.full(1, 12345, dtype=U64)])
    chunks = [
        ("update", upd, upd ^ U64(0x5A5A5A)),
        ("delete", dele, np.zeros(dele.size, dtype=U64)),
        ("reinsert", dele, dele ^ U64(0xC3C3C3)),
        ("delete2", k_first, np.zeros(k_first.size, dtype=U64)),
        ("mixed", mix_k, mix_v),
        ("new", new, new ^ U64(0x1234567)),
        ("split", runs, runs ^ U64(0x77)),
    ]
    for name, k, v in chunks:
        splits0 = t.stats()["splits"]
        t.insert_batch(dev(k), dev(v))
        orc.apply_batch(k, v)
        stored, _ = orc.dump()
        touched = np.unique(np.concatenate([k, Buckets(t, stored).members(np.unique(bk.of(k))),
                                            k + U64(1), sample]))
        touched = touched[touched != U64(shm.KEY_MAX)]
        touched = np.unique(np.append(touched, U64(0)))
        gv, gf, s = gpu_search_stats(t, touched)
        assert_same(touched, *orc.search_batch(touched), gv, gf)
        model_clean(t, orc)
        vs = t.vt_stats()
        print(name, s, vs)
        assert vs["trusted"], (name, vs)
        assert t.dir_stats()["builds"] == builds, (name, t.dir_stats())
        assert t.last_error()["bits"] == 0, name
        buckets, _ = t.vt_dump()
        d = vm.dead(buckets)
        if name == "reinsert":  # the tombstones were reused: no key twice, dead or live
            sk, sv = buckets[:, 0::2], buckets[:, 1::2]
            rows = bk.of(dele)
            assert ((sk[rows] == dele[:, None]).sum(axis=1) == 1).all()
            assert ((sk[rows] == dele[:, None]) & (sv[rows] != 0)).sum() == dele.size
        if name == "new":
            assert d[full].all() and not d[by_count[7][:300]].any()
        if name == "mixed":  # key 0 is stored, and no bucket holds it
            assert gf[0] == 1 and int(gv[0]) == 12345 and touched[0] == 0
            assert not d[mix_b].any()
        if name == "split":
            assert d[empty].all()
            # the runs did split leaves: the upkeep kept the table beside splits
            assert t.stats()["splits"] >= splits0 + empty.size // 2, (splits0, t.stats())
    rc, oc = orc.check()
    assert rc == 0 and t.check()["keys"] == oc["keys"]
    orc.close()
    t.close()


@pytest.mark.parametrize("how", ["off", "unsearched"])
def test_chunks_without_upkeep_end_the_trust(lib_ok, how):
    """A chunk that is not kept -- the upkeep switched off after the build,
    or the default policy's chunk with no search before it -- leaves the
    table behind the tree: it is untrusted from then on and the gets do not
    read it: updated and deleted keys equal the oracle."""
    t, orc, base = loaded(maint="always" if how == "off" else True)
    assert t.vt_stats()["trusted"]
    rng = np.random.default_rng(33)
    pick = rng.permutation(N0)
    upd, dele = base[pick[:4000]], base[pick[4000:8000]]
    if how == "off":
        t.dir_config(maint=False)
    else:  # a searched chunk is kept; the next one, unsearched, is not
        warm = base[pick[8000:8100]]
        t.insert_batch(dev(warm), dev(warm ^ U64(3)))
        orc.apply_batch(warm, warm ^ U64(3))
        assert t.vt_stats()["trusted"]
    k = np.concatenate([upd, dele])
    v = np.concatenate([upd ^ U64(0xABCDEF), np.zeros(dele.size, dtype=U64)])
    t.insert_batch(dev(k), dev(v))
    orc.apply_batch(k, v)
    assert not t.dir_stats()["exact"]
    assert not t.vt_stats()["trusted"]
    probe = np.concatenate([k, base[pick[8000:12000]]])
    gv, gf = gpu_search(t, probe)
    assert_same(probe, *orc.search_batch(probe), gv, gf)
    assert not t.vt_stats()["trusted"]
    orc.close()
    t.close()


@pytest.mark.parametrize("switch", ["SHM_VALTAB", "SHM_DIR_VALS", "page_check"])
def test_switches_read_every_hit_from_its_leaf(lib_ok, switch):
    """SHM_VALTAB=0, SHM_DIR_VALS=0 and SHM_FLAG_PAGE_CHECK never read the
    table: stored probes read at least one leaf entry per hit.  With
    SHM_VALTAB=0 alone the directory's value form still answers the prefixes
    of at most two keys from the entry, as before the table, so there the
    probes are keys whose prefix holds more than two keys (95 % of them
    would read no entry with the table on); the other two switches take any
    stored key."""
    if switch == "page_check":
        t, orc, base = loaded(page_check=True)
    else:
        t, orc, base = without_table(loaded) if switch == "SHM_VALTAB" else with_env(switch, "0", loaded)
    vs = t.vt_stats()
    assert vs["buckets"] == 0 or switch == "page_check", vs
    ent = t.dir_stats()["entries"]
    pref = (base >> U64(64 - (ent.bit_length() - 1))).astype(np.int64)
    held = np.bincount(pref, minlength=ent)[pref]
    big = base[held > 2] if switch == "SHM_VALTAB" else base
    rng = np.random.default_rng(34)
    probe = np.concatenate([big[rng.integers(0, big.size, 1 << 15)],
                            gen_keys(t, N0 + 1, 1 << 12)])
    gv, gf, st = gpu_search_stats(t, probe)
    assert_same(probe, *orc.search_batch(probe), gv, gf)
    assert st["hits"] == 1 << 15 and st["entry_reads"] >= st["hits"], st
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


def test_ordering_on_a_second_stream_does_not_reach_the_table_upkeep(lib_ok):
    """The scheme of test_ordering_on_a_second_stream_does_not_reach_the_upkeep
    at chunks of 2^14: eight rounds of insert_order(i + 1) on stream B, a
    search on stream A, insert_apply(i) on A, with new keys and updates.
    Every search equals the oracle's state at that point and the table's
    model is clean at the end."""
    mb = 1 << 14
    t, orc, base = loaded(max_batch=mb)
    bk = Buckets(t, base)
    rng = np.random.default_rng(35)
    builds = t.dir_stats()["builds"]
    populated = np.nonzero((bk.count >= 1) & (bk.count <= 6))[0]
    stored = base
    batches = []
    for r in range(9):
        new = bk.fresh_in(rng.permutation(populated)[:6000], rng, stored)
        upd = np.unique(base[rng.integers(0, N0, 6000)])
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
    assert t.vt_stats()["trusted"]
    model_clean(t, orc)
    assert t.dir_stats()["builds"] == builds
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


def test_dense_keys_drop_the_table(lib_ok):
    """2^17 dense keys 1 .. 2^17 under the default 64-bit range all land in
    one bucket: the build finds (almost) every key in a dead bucket and the
    table is dropped; 2^17 hashed keys through the same path keep theirs.
    Both sets' gets equal the oracle."""
    n = 1 << 17
    dense = np.arange(1, n + 1, dtype=U64)
    t, orc, _ = loaded(keys=dense)
    vs = t.vt_stats()
    assert vs["buckets"] == 0 and not vs["trusted"], vs
    rng = np.random.default_rng(36)
    probe = np.concatenate([dense[rng.integers(0, n, 1 << 14)],
                            np.arange(n + 1, n + 1025, dtype=U64)])
    gv, gf = gpu_search(t, probe)
    assert_same(probe, *orc.search_batch(probe), gv, gf)
    assert t.vt_stats()["buckets"] == 0
    orc.close()
    t.close()
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 18)
    hashed = gen_keys(t, 1, n)
    t.close()
    t, orc, _ = loaded(keys=hashed)
    vs = t.vt_stats()
    assert vs["trusted"] and vs["buckets"] > 0, vs
    probe = np.concatenate([hashed[rng.integers(0, n, 1 << 14)], dense[:1024]])
    gv, gf = gpu_search(t, probe)
    assert_same(probe, *orc.search_batch(probe), gv, gf)
    model_clean(t, orc)
    orc.close()
    t.close()


def test_memory_limit_leaves_no_table(lib_ok):
    """The table's bytes count against the directory's memory limit: with
    the limit at the directory's own bytes there is no table, the directory
    is what it was, and the gets equal the oracle."""
    t, orc, base = loaded()
    d0 = t.dir_stats()
    assert t.vt_stats()["buckets"] > 0
    orc.close()
    t.close()
    t, orc, base = loaded(mem_limit=d0["bytes"])
    d1 = t.dir_stats()
    assert d1["bytes"] == d0["bytes"] and d1["entries"] == d0["entries"], (d0, d1)
    vs = t.vt_stats()
    assert vs["buckets"] == 0 and not vs["trusted"], vs
    rng = np.random.default_rng(37)
    probe = base[rng.integers(0, N0, 1 << 14)]
    gv, gf = gpu_search(t, probe)
    assert_same(probe, *orc.search_batch(probe), gv, gf)
    orc.close()
    t.close()
