"""Ordered scans with a count limit (shm_scan_batch, Tree.scan_batch /
lower_bound_batch) on the GPU against the numpy model (tests/scan_model.py)
over the CPU oracle's contents.

Every check compares counts, keys and values exactly with the model, asserts
that the words of a scan's row past its count still hold the sentinel the
buffers were filled with, and that the device error bits are zero.  The trees
are small (20,000 keys are about 600 leaves under a level-2 root), which is
enough for every path of the kernel: the directory start and the descent from
the root, B-link right turns, leaves with holes and unsorted slots, the limit
cut at every position of a leaf, and the `to` bound.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, host, lib_ok, SENT, U64  # noqa: E402
from oracle.pyoracle import OracleTree, to_key  # noqa: E402
from scan_model import KEY_MAX, ScanModel  # noqa: E402

ARENA = 64 << 20
TOP = 1 << 63


def hashed_keys(lo, hi):
    return np.array([to_key(i) for i in range(lo, hi)], dtype=U64)


def put(t, orc, keys, vals):
    """One batch into both trees (value 0 deletes)."""
    t.insert_batch(dev(keys), dev(vals))
    orc.apply_batch(keys, vals)


def queue_scans(t, lo, limit, hi=None):
    """Queues the scans into sentinel-filled buffers; returns what check_scans
    needs.  status[0] is set to a mark the call must leave alone."""
    n = lo.size
    keys = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
    vals = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
    counts = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    status = torch.tensor([77, 0], dtype=torch.int64, device="cuda")
    d_lo = dev(lo)
    d_hi = None if hi is None else dev(hi)
    pend = t.scan_batch(d_lo, limit, hi=d_hi, keys=keys, vals=vals, counts=counts, status=status)
    return pend, status, (d_lo, d_hi)


def check_scans(model, queued, lo, limit, hi=None):
    pend, status, _ = queued
    c, k, v = pend.result()
    assert status.cpu().tolist() == [77, 0], status
    c, k, v = c.cpu().numpy(), host(k), host(v)
    mc, mk, mv, w = model.scan(lo, limit, hi)
    bad = np.nonzero(c != mc)[0]
    assert bad.size == 0, (f"{bad.size} counts differ, first: scan {bad[0]} lo={int(lo[bad[0]]):#x} "
                           f"limit={limit} gpu={c[bad[0]]} model={mc[bad[0]]}")
    assert k.shape == mk.shape == (lo.size, limit)
    for name, g, m in (("key", k, mk), ("value", v, mv)):
        ne = np.argwhere(w & (g != m))
        assert ne.size == 0, (f"{name}s differ at {len(ne)} places, first: scan {ne[0][0]} "
                              f"lo={int(lo[ne[0][0]]):#x} limit={limit} pos {ne[0][1]} "
                              f"gpu={int(g[tuple(ne[0])]):#x} model={int(m[tuple(ne[0])]):#x}")
        assert (g[~w] == U64(SENT)).all(), f"{name} row tails were written (limit {limit})"
    return mc, mk, mv


def scan_and_check(t, model, lo, limit, hi=None):
    lo = np.ascontiguousarray(lo, dtype=U64)
    if hi is not None:
        hi = np.ascontiguousarray(hi, dtype=U64)
    out = check_scans(model, queue_scans(t, lo, limit, hi), lo, limit, hi)
    assert t.last_error()["bits"] == 0
    return out


def froms_around(model):
    """Every 37th stored key, those keys +- 1, 0, below the minimum, above the
    maximum, KEY_MAX - 1 and KEY_MAX."""
    s = model.keys[::37]
    return np.concatenate([s, s + U64(1), s - U64(1),
                           np.array([0, int(model.keys[0]) - 1, int(model.keys[-1]) + 1,
                                     KEY_MAX - 1, KEY_MAX], dtype=U64)])


@pytest.mark.parametrize("leaf_dir", [True, False])
def test_churned_tree_against_the_model(lib_ok, leaf_dir):
    """20,000 hashed keys, then three rounds of deletes (value 0), overwrites
    and re-inserts, mirrored into the oracle: leaves with holes and with slots
    out of key order.  After each round every limit from every `from`."""
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
        # half of the deleted keys come back, beside as many new ones: they
        # take the first empty slots, wherever those are
        back = np.concatenate([dele[:1500], hashed_keys(30001 + 1500 * r, 31501 + 1500 * r)])
        put(t, orc, back, back ^ U64(0x7700 + r))
        model = ScanModel.of(orc)
        assert model.keys.size == t.check()["keys"]
        lo = froms_around(model)
        for limit in (1, 2, 7, 53, 54, 55, 200):
            mc, mk, _ = scan_and_check(t, model, lo, limit)
            last = mk[np.arange(lo.size), np.maximum(mc, 1) - 1]
            crossed += int(((mc > 0) & (lo < U64(TOP)) & (last >= U64(TOP))).sum())
    assert (base < U64(TOP)).any() and (base >= U64(TOP)).any()
    assert crossed > 0, "no scan's result crossed 2^63"
    orc.close()
    t.close()


class Dense:
    """3,000 dense keys 3 * i (i = 1 .. 3000) inserted in a random permutation, then every
    fifth deleted: read-only after the build."""

    def __init__(self, leaf_dir):
        self.t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 12, leaf_dir=leaf_dir)
        self.orc = OracleTree(ARENA)
        rng = np.random.default_rng(43)
        ks = np.arange(1, 3001, dtype=U64) * U64(3)
        dele = ks[::5].copy()
        ks = ks[rng.permutation(ks.size)]
        # several batches: later keys land in the first empty slot of leaves
        # the earlier ones made, so slot order is not key order
        for c in range(0, ks.size, 500):
            put(self.t, self.orc, ks[c:c + 500], ks[c:c + 500] + U64(7))
        put(self.t, self.orc, dele, np.zeros(dele.size, dtype=U64))
        self.model = ScanModel.of(self.orc)
        assert self.model.keys.size == 2400 == self.t.check()["keys"]


@pytest.fixture(scope="module", params=[True, False], ids=["dir", "nodir"])
def dense(request, lib_ok):
    d = Dense(request.param)
    yield d
    d.orc.close()
    d.t.close()


def test_every_alignment_against_leaf_ends(dense):
    """`from` at every stored key and every key + 1, unbounded: the limit cut
    falls at each position inside a leaf and at each leaf boundary without
    the test knowing the fences."""
    s = dense.model.keys
    lo = np.concatenate([s, s + U64(1)])
    for limit in (1, 54, 55, 108):
        scan_and_check(dense.t, dense.model, lo, limit)


def test_the_to_bound(dense):
    t, model, orc = dense.t, dense.model, dense.orc
    s = model.keys
    absent = s + U64(1)  # stored keys are multiples of 3
    i = np.arange(0, s.size - 80, 7)
    cases = [
        (s[1:], s[1:] - U64(1), 0),                    # to < from
        (s, s, 1),                                     # to == from on a stored key
        (absent, absent, 0),                           # to == from on an absent key
        (s[i], s[i + 5] + U64(1), 6),                  # to between two stored keys
        (s[i] + U64(1), s[i + 5] - U64(1), 4),
        (s[i], s[i + 70] + U64(1), 71),                # ends the scan before limit 108, leaves apart
        (s[i] + U64(2), s[i + 70], 70),
    ]
    for limit in (1, 54, 108):
        for lo, hi, want in cases:
            mc, _, _ = scan_and_check(t, model, lo, limit, hi)
            assert (mc == min(want, limit)).all(), (limit, want)
    # bounded scans below the limit hold the same values as the reference's
    # range_query (any order there)
    lo, hi = s[i], s[i + 70] + U64(1)
    pend, status, _ = queue_scans(t, lo, 108, hi)
    c, _, v = pend.result()
    c, v = c.cpu().numpy(), host(v)
    assert (c == 71).all()
    for j in range(lo.size):
        ref, n = orc.range_query(int(lo[j]), int(hi[j]), cap=4096)
        assert n == c[j] and np.array_equal(np.sort(ref), np.sort(v[j, :n])), j


def test_stale_directory(lib_ok):
    """Leaves split behind a directory that is not rebuilt: scans that start
    on a split leaf reach their keys by B-link right turns.  2^16 hashed keys
    in two chunks (at one chunk every leaf holds 36 keys, each of the 60
    splits adds a page, and 60 pages are more than the 1/32 the directory
    tolerates of about 1,870)."""
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
    model = ScanModel.of(orc)
    lo = np.concatenate([anchors - U64(1), anchors])
    for limit in (1, 40, 120):
        scan_and_check(t, model, lo, limit)
    pages1 = t.stats()["pages_used"]
    d1 = t.dir_stats()
    print("stale directory: pages", pages0, "->", pages1, d1)
    # the condition of the test: leaves split, and the directory is the old one
    assert pages0 + 20 <= pages1 < pages0 + pages0 // 32, (pages0, pages1)
    assert d1["builds"] == d0["builds"], (d0, d1)
    orc.close()
    t.close()


@pytest.mark.parametrize("leaf_dir", [True, False])
def test_empty_tree_and_empty_batch(lib_ok, leaf_dir):
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 12, leaf_dir=leaf_dir)
    model = ScanModel(np.zeros(0, dtype=U64), np.zeros(0, dtype=U64))
    lo = np.array([0, 1, 12345, TOP, KEY_MAX - 1, KEY_MAX], dtype=U64)
    for limit in (1, 60):
        mc, _, _ = scan_and_check(t, model, lo, limit)
        assert (mc == 0).all()
        scan_and_check(t, model, lo, limit, hi=np.full(lo.size, KEY_MAX, dtype=U64))
    # n == 0: SHM_OK (no exception), nothing launched, nothing written
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    keys = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    vals = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    counts = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    status = torch.tensor([77, 0], dtype=torch.int64, device="cuda")
    c, k, v = t.scan_batch(e, 4, keys=keys, vals=vals, counts=counts, status=status).result()
    assert c.numel() == 0 and tuple(k.shape) == (0, 4) and tuple(v.shape) == (0, 4)
    assert status.cpu().tolist() == [77, 0]
    for b in (keys, vals, counts):
        assert (host(b) == U64(SENT)).all()
    c, k, v = t.scan_batch(e, 3, hi=e).result()
    assert c.numel() == 0
    found, k1, v1 = t.lower_bound_batch(e)
    assert found.numel() == k1.numel() == v1.numel() == 0
    assert t.last_error()["bits"] == 0
    t.close()


@pytest.mark.parametrize("leaf_dir", [True, False])
def test_stream_order(lib_ok, leaf_dir):
    """scan, insert_batch_async of keys inside the scans' windows, scan, all
    queued on one stream with no wait between them: the first scan sees the
    tree before the insert, the second the tree after it."""
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 15, leaf_dir=leaf_dir)
    orc = OracleTree(ARENA)
    base = hashed_keys(1, 20001)
    put(t, orc, base, base ^ U64(0x4444))
    before = ScanModel.of(orc)
    lo = before.keys[::61].copy()
    ins = np.concatenate([lo + U64(1), lo + U64(2), before.keys[5::61]])  # new keys and overwrites
    iv = ins ^ U64(0x5555)
    limit = 20
    s = torch.cuda.current_stream()
    q1 = queue_scans(t, lo, limit)
    dk, dv = dev(ins), dev(iv)
    t.insert_batch_async(dk, dv, stream=s)
    q2 = queue_scans(t, lo, limit)
    orc.apply_batch(ins, iv)
    after = ScanModel.of(orc)
    _, k1, _ = check_scans(before, q1, lo, limit)
    _, k2, _ = check_scans(after, q2, lo, limit)
    assert not np.array_equal(k1, k2)  # the insert lies inside the windows
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


@pytest.mark.parametrize("leaf_dir", [True, False])
def test_lower_bound_batch_against_searchsorted(lib_ok, leaf_dir):
    t = shm.Tree(arena_bytes=ARENA, max_batch=1 << 15, leaf_dir=leaf_dir)
    base = hashed_keys(1, 20001)
    vals = base ^ U64(0x6666)
    t.insert_batch(dev(base), dev(vals))
    order = np.argsort(base)
    sk, sv = base[order], vals[order]
    probe = np.concatenate([sk[::3], sk[::5] + U64(1), sk[::7] - U64(1),
                            np.array([0, int(sk[0]) - 1, int(sk[-1]) + 1, KEY_MAX - 1, KEY_MAX],
                                     dtype=U64)])
    found, k, v = t.lower_bound_batch(dev(probe))
    found, k, v = found.cpu().numpy(), host(k), host(v)
    idx = np.searchsorted(sk, probe, side="left")
    want = idx < sk.size
    assert want[:-3].all() and not want[-3:].any()
    assert np.array_equal(found, want)
    assert np.array_equal(k[want], sk[idx[want]]) and np.array_equal(v[want], sv[idx[want]])
    assert (k[~want] == 0).all() and (v[~want] == 0).all()
    assert (probe < U64(TOP)).any() and (k >= U64(TOP)).any()
    assert t.last_error()["bits"] == 0
    t.close()
