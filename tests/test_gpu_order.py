"""The insert ordering on every path (isort.hip, partition.hip's coarse pass),
read back before the apply stage can mask it.

Each case (tests/order_cases.py): the batch, its path asserted by
order_model.plan, insert_order, then Tree.order_read -- counts, uk, uv and dk
as insert_apply will read them -- compared exactly with order_model.order;
then insert_apply, and the tree's export against the contents before the
chunk updated by it, Tree.check() and the error word.  The trees are shared
by the cases of the module, so deletes and overwrites meet stored keys; each
case reads the contents it starts from off the tree.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import order_cases as oc  # noqa: E402
import order_model as om  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, host, U64  # noqa: E402

KEY_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def lim():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return shm.order_limits()


@pytest.fixture(scope="module")
def trees(lim):
    ts = {"small": shm.Tree(arena_bytes=128 << 20, max_batch=1 << 14),
          "big": shm.Tree(arena_bytes=1 << 30, max_batch=1 << 22)}
    # a stored image to start from: half of the keys the spread cases draw
    for name, n in (("small", 1 << 13), ("big", 1 << 19)):
        k = oc.splitmix(np.arange(0, n, 2))
        ts[name].insert_batch(dev(k), dev(k | U64(1)))
    yield ts
    for t in ts.values():
        t.close()


def contents(t):
    k, v = t.export()
    return host(k).copy(), host(v).copy()


def same(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, bad.size, int(bad[0]), hex(int(got[bad[0]])),
                           hex(int(want[bad[0]])))


def queue_order(t, keys, vals):
    """insert_order: the ticket, and the device tensors to keep alive until
    the ordering has run"""
    kd, vd = dev(keys), dev(vals)
    tk = t.insert_order(kd, vd)
    assert tk != 0
    return tk, (kd, vd)


def read_exact(t, tk, keys, vals, what):
    """order_read of the ticket equals the model's ordering of the chunk"""
    uk, uv, dk, counts = t.order_read(tk, keys.size)
    euk, euv, edk = om.order(keys, vals)
    assert counts == (euk.size, edk.size), (what, counts, euk.size, edk.size)
    same(uk, euk, what + ": uk")
    same(uv, euv, what + ": uv")
    same(dk, edk, what + ": dk")
    return euk, euv, edk


def applied(t, before, chunks, what):
    """the tree after the chunks (already queued): the export equals the
    image before them updated by each in turn"""
    t.synchronize()
    k, v = before
    for c in chunks:
        k, v = om.apply(k, v, *c)
    gk, gv = contents(t)
    same(gk, k, what + ": exported keys")
    same(gv, v, what + ": exported values")
    assert t.check()["keys"] == k.size, what
    assert t.last_error()["bits"] == 0, (what, t.last_error())
    return k, v


@pytest.mark.parametrize("name", list(oc.BUILDERS))
def test_ordered_chunk(trees, lim, name):
    c = oc.BUILDERS[name](lim)
    t = trees[c.tree]
    lo, bits = c.hint or (0, 64)
    c.expect(om.plan(c.keys, lo, bits, lim))  # the path this batch is for
    if c.hint:
        t.set_key_range(lo, bits)
    try:
        before = contents(t)
        tk, keep = queue_order(t, c.keys, c.vals)
        exp = read_exact(t, tk, c.keys, c.vals, name)
        if c.counts is not None:
            assert (exp[0].size, exp[2].size) == c.counts
        if name == "all_deletes":
            assert exp[0].size == 0 and np.isin(exp[2], before[0]).any()
        if name == "no_deletes":
            assert exp[2].size == 0 and np.isin(exp[0], before[0]).any()
        t.insert_apply(tk)
        applied(t, before, [exp], name)
        del keep
    finally:
        if c.hint:
            t.synchronize()
            t.set_key_range(0, 64)


def test_key_bits_zero_is_the_whole_key_space(trees):
    """hint_1 is the narrowest hint; shm_tree_set_key_range also takes 0,
    which it reads as 64 with key_lo 0: nothing clamps"""
    t = trees["small"]
    t.set_key_range(oc.HINT_LO, 0)
    try:
        k = np.array([5, oc.HINT_LO + 9], dtype=U64)
        p = om.plan(k, oc.HINT_LO, 0, shm.order_limits())
        assert p.cnt[0] == 2  # the whole key space: both in bin 0, nothing clamps
        before = contents(t)
        v = np.array([70, 71], dtype=U64)
        tk, keep = queue_order(t, k, v)
        exp = read_exact(t, tk, k, v, "bits 0")
        t.insert_apply(tk)
        applied(t, before, [exp], "bits 0")
    finally:
        t.set_key_range(0, 64)


def test_two_tickets_outstanding(trees, lim):
    """order A, order B (the other parity's buffers), read both, apply both:
    B's ordering leaves A's ordered chunk as it was"""
    t = trees["small"]
    rng = np.random.default_rng(2024)
    n = 3 * lim["tile"] + 11
    ka = oc.spread(rng, n, n // 2)
    kb = oc.spread(rng, n, n // 2)
    kb[:500] = ka[-500:]  # B overwrites and deletes what A writes
    va, vb = oc.values("two_a", rng, n), oc.values("two_b", rng, n)
    before = contents(t)
    ta, keep_a = queue_order(t, ka, va)
    tb, keep_b = queue_order(t, kb, vb)
    assert (ta ^ tb) & 1
    with pytest.raises(shm.ShermanError) as e:
        t.insert_order(*keep_a)  # no third
    assert e.value.rc == shm.SHM_EAGAIN
    ea = read_exact(t, ta, ka, va, "A")
    eb = read_exact(t, tb, kb, vb, "B")
    ea2 = read_exact(t, ta, ka, va, "A again")  # a read changes nothing
    assert all(np.array_equal(x, y) for x, y in zip(ea, ea2))
    with pytest.raises(shm.ShermanError) as e:
        t.order_read(tb + 1, n)  # not outstanding
    assert e.value.rc == shm.SHM_EINVAL
    t.insert_apply(ta)
    with pytest.raises(shm.ShermanError) as e:
        t.order_read(ta, n)  # applied
    assert e.value.rc == shm.SHM_EINVAL
    eb = read_exact(t, tb, kb, vb, "B after A's apply")
    t.insert_apply(tb)
    applied(t, before, [ea, eb], "A then B")


def test_padded_slots(trees, lim):
    """one shm__insert_batch_padded call: KEY_MAX slots among the ops, a
    whole tile of padding (gcount == 0), the last tile partly padded; the
    tree gets the unpadded ops and no error bit"""
    t = trees["small"]
    T = lim["tile"]
    rng = np.random.default_rng(77)
    n = 4 * T - 300
    keys = oc.spread(rng, n, 2000)
    vals = oc.values("padded", rng, n)
    pad = np.zeros(n, dtype=bool)
    pad[:T] = rng.random(T) < 0.4       # interleaved
    pad[T:2 * T] = True                  # nothing but padding
    pad[3 * T + 900:] = True             # the last tile's tail
    pad[3 * T + 100:3 * T + 200] = True
    keys[pad] = KEY_MAX
    vals[pad] = rng.integers(0, 5, int(pad.sum()), dtype=np.uint64)  # never read
    p = om.plan(keys, 0, 64, lim, skip_pad=True)
    assert p.mode == "tile" and p.tiles == 4 and p.cnt.sum() > 0
    before = contents(t)
    kd, vd = dev(keys), dev(vals)
    t.insert_batch_padded(kd, vd)
    exp = om.order(keys[~pad], vals[~pad])
    assert exp[0].size and exp[2].size and np.isin(exp[2], before[0]).any()
    applied(t, before, [exp], "padded")


@pytest.mark.parametrize("which", ["small", "big"])
def test_empty_chunk(trees, lim, which):
    """include/sherman_amd.h: n == 0 takes no chunk id and queues nothing,
    the ticket is 0 and its apply is accepted at any time.  (The big tree
    has run coarse passes by now: their bin table stays behind, which an
    empty ordering must not read.)"""
    t = trees[which]
    before = contents(t)
    last = t.last_chunk()
    e0 = torch.empty(0, dtype=torch.int64, device="cuda")
    assert t.insert_order(e0, e0) == 0
    with pytest.raises(shm.ShermanError) as e:
        t.order_read(0, 0)
    assert e.value.rc == shm.SHM_EINVAL
    t.insert_apply(0)
    # beside an outstanding ticket, which stays as it is
    rng = np.random.default_rng(5)
    k, v = oc.spread(rng, 3000, 1500), oc.values("empty", rng, 3000)
    tk, keep = queue_order(t, k, v)
    assert t.insert_order(e0, e0) == 0
    t.insert_apply(0)
    exp = read_exact(t, tk, k, v, "A beside an empty chunk")
    t.insert_apply(tk)
    assert t.last_chunk() == last + 1
    applied(t, before, [exp], "A")
    t.insert_batch(e0, e0)
    assert t.last_chunk() == last + 1
    applied(t, before, [exp], "empty insert_batch")
