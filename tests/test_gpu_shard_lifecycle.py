"""The C-ABI shard handle's lifecycle and the statuses of its misuse, on one
GPU through the in-process group (shm__shard_create_local).

The routed paths themselves are tests/test_gpu_shard_local.py's; this file
pins what surrounds them and what no other test looks at: which status each
refused call returns (and that a refused call leaves the handle usable), that
a handle can be closed and a second one opened on the same tree, and that a
creation which fails after everything was allocated (two ranks whose trees
have different max_batch: SHM_EINVAL from the one exchange at creation)
releases the handle and leaves the trees and the group usable.

Trees of max_batch 1024 with small arenas: every case takes seconds.
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U64 = np.uint64
MAX_BATCH = 1024
ARENA = 16 << 20


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).to("cuda:0")


def rc_of(call, *args, **kw):
    """The status a wrapper call raises (0 when it returns)."""
    import sherman_amd as shm
    try:
        call(*args, **kw)
    except shm.ShermanError as e:
        return e.rc
    return 0


def shard_get(cs, q):
    vals = torch.empty(q.size, dtype=torch.int64, device="cuda:0")
    found = torch.empty(q.size, dtype=torch.uint8, device="cuda:0")
    cs.search(dev_u64(q), vals, found)
    torch.cuda.synchronize()
    return vals.cpu().numpy().view(U64), found.cpu().numpy()


def test_world1_statuses_and_reopen():
    import sherman_amd as shm
    from oracle.pyoracle import OracleTree

    assert torch.cuda.is_available(), "GPU test without a GPU"
    torch.cuda.set_device(0)
    L = shm.lib()
    rng = np.random.default_rng(20)
    keys = np.unique(rng.integers(1, (1 << 64) - 2, 900, dtype=U64))[:800]
    vals = rng.integers(1, 1 << 40, keys.size, dtype=U64)
    ref = OracleTree(ARENA)
    tree = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, device=0)
    tree.insert_batch(dev_u64(keys[:600]), dev_u64(vals[:600]))
    ref.apply_batch(keys[:600], vals[:600])
    group = shm.LocalGroup(1)
    cs = shm.CShard.local(tree, group, 0)

    # nothing to copy out before the first range query
    assert L.shm_shard_range_values(cs.h, None, 0, None) == shm.SHM_EINVAL
    big = dev_u64(np.arange(1, MAX_BATCH + 2))
    assert rc_of(cs.search_begin, big) == shm.SHM_E2BIG
    assert rc_of(cs.range_query, dev_u64([1]), dev_u64([2]), n_cap=MAX_BATCH + 1) == shm.SHM_E2BIG
    assert L.shm_shard_range_values(cs.h, None, 0, None) == shm.SHM_EINVAL

    # two batches begun (hits and misses), every slot busy
    q = [np.concatenate([keys[:300], keys[700:750]]), np.concatenate([keys[650:800], keys[200:500]])]
    qd = [dev_u64(x) for x in q]
    t0 = cs.search_begin(qd[0])
    t1 = cs.search_begin(qd[1])
    assert (t0, t1) == (0, 1)
    assert rc_of(cs.search_begin, qd[0]) == shm.SHM_EINVAL
    assert rc_of(cs.set_splitters, None) == shm.SHM_EINVAL
    assert rc_of(cs.rebalance) == shm.SHM_EINVAL
    out = [(torch.empty(x.size, dtype=torch.int64, device="cuda:0"),
            torch.empty(x.size, dtype=torch.uint8, device="cuda:0")) for x in q]
    assert rc_of(cs.search_end, 2, *out[0]) == shm.SHM_EINVAL
    # the refused calls took nothing from the begun batches
    cs.search_end(t0, *out[0])
    assert rc_of(cs.search_end, t0, *out[0]) == shm.SHM_EINVAL  # ended already
    cs.search_end(t1, *out[1])
    torch.cuda.synchronize()
    for x, (v, f) in zip(q, out):
        ov, of = ref.search_batch(x)
        assert np.array_equal(v.cpu().numpy().view(U64), ov)
        assert np.array_equal(f.cpu().numpy(), of)

    # an insert (new keys, overwrites, a delete) and a get of what it wrote
    ik = np.concatenate([keys[600:800], keys[:50]])
    iv = np.concatenate([vals[600:800], vals[:50] + U64(7)])
    iv[-1] = 0
    cs.insert(dev_u64(ik), dev_u64(iv))
    cs.synchronize()
    ref.apply_batch(ik, iv)
    probe = np.concatenate([keys, rng.integers(1, (1 << 64) - 2, 40, dtype=U64)])
    ov, of = ref.search_batch(probe)
    gv, gf = shard_get(cs, probe)
    assert np.array_equal(gv, ov) and np.array_equal(gf, of)

    # close, a second handle on the same tree, the same get
    cs.close()
    cs = shm.CShard.local(tree, group, 0)
    gv, gf = shard_get(cs, probe)
    assert np.array_equal(gv, ov) and np.array_equal(gf, of)
    cs.close()
    group.close()
    assert tree.check()["keys"] >= 0
    tree.close()
    ref.close()


def create_rank(r, trees, group, stream, out, errs):
    import sherman_amd as shm
    try:
        with torch.cuda.stream(stream):
            try:
                out[r] = shm.CShard.local(trees[r], group, r)
            except shm.ShermanError as e:
                out[r] = e.rc
    except BaseException as e:  # noqa: BLE001 - reported by the main thread
        errs.append((r, repr(e)))


def routed_rank(r, shards, stream, batches, queries, out, errs):
    try:
        with torch.cuda.stream(stream):
            cs = shards[r]
            cs.insert(dev_u64(batches[r][0]), dev_u64(batches[r][1]), stream=stream)
            vals = torch.empty(queries[r].size, dtype=torch.int64, device="cuda:0")
            found = torch.empty(queries[r].size, dtype=torch.uint8, device="cuda:0")
            cs.search(dev_u64(queries[r]), vals, found, stream=stream)
            cs.synchronize()
            stream.synchronize()
            out[r] = (vals.cpu().numpy().view(U64), found.cpu().numpy())
            cs.close()
    except BaseException as e:  # noqa: BLE001 - reported by the main thread
        errs.append((r, repr(e)))


def run_threads(target, world, *args):
    out, errs = [None] * world, []
    th = [threading.Thread(target=target, args=(r,) + args + (out, errs)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank thread hung"
    assert not errs, errs
    return out


def test_world2_failed_creation_releases_everything():
    import sherman_amd as shm
    from oracle.pyoracle import OracleTree
    from sherman_amd.shard import shard_range

    assert torch.cuda.is_available(), "GPU test without a GPU"
    torch.cuda.set_device(0)
    P = 2
    rng = np.random.default_rng(21)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())

    def make_trees(caps):
        ts = []
        for r, cap in enumerate(caps):
            lo, bits = shard_range(r, P)
            ts.append(shm.Tree(arena_bytes=ARENA, max_batch=cap, device=0, node_id=r, key_lo=lo,
                               key_bits=bits))
        return ts

    # each rank's own keys (top bit = rank), written locally
    own = [(U64(r) << U64(63)) | rng.integers(1, (1 << 63) - 2, 200, dtype=U64) for r in range(P)]
    trees = make_trees([MAX_BATCH, 2 * MAX_BATCH])
    for r, t in enumerate(trees):
        t.insert_batch(dev_u64(own[r]), dev_u64(own[r] ^ U64(0x55)))
    group = shm.LocalGroup(P)
    got = run_threads(create_rank, P, trees, group, stream)
    assert got == [shm.SHM_EINVAL, shm.SHM_EINVAL], got  # the caps differ: both ranks refuse
    torch.cuda.synchronize()
    for r, t in enumerate(trees):
        v = torch.empty(own[r].size, dtype=torch.int64, device="cuda:0")
        f = torch.empty(own[r].size, dtype=torch.uint8, device="cuda:0")
        t.search_batch(dev_u64(own[r]), v, f)
        torch.cuda.synchronize()
        assert np.array_equal(v.cpu().numpy().view(U64), own[r] ^ U64(0x55))
        assert bool(f.all())
        t.close()
    group.close()

    # equal caps on fresh trees: the group forms and routes
    trees = make_trees([MAX_BATCH, MAX_BATCH])
    group = shm.LocalGroup(P)
    shards = run_threads(create_rank, P, trees, group, stream)
    assert all(isinstance(s, shm.CShard) for s in shards), shards
    ref = OracleTree(ARENA)
    # every rank writes keys of both shards; 64 gets per rank, some misses
    pool = np.unique(rng.integers(1, (1 << 64) - 2, 600, dtype=U64))
    batches, queries = [], []
    for r in range(P):
        k = pool[r::P][:250]
        batches.append((k, k ^ U64(0x1234 + r)))
        queries.append(np.concatenate([pool[rng.integers(0, 500, 56)],
                                       rng.integers(1, (1 << 64) - 2, 8, dtype=U64)]))
        ref.apply_batch(*batches[r])
    res = run_threads(routed_rank, P, shards, stream, batches, queries)
    for r in range(P):
        ov, of = ref.search_batch(queries[r])
        assert np.array_equal(res[r][0], ov), r
        assert np.array_equal(res[r][1], of), r
    ref.close()
    group.close()
    for t in trees:
        assert t.check()["keys"] >= 0
        t.close()
