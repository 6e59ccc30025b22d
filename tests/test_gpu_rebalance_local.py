"""shm_shard_rebalance in the in-process group on one GPU (the set-up of
test_gpu_shard_local.py: P trees on cuda:0, one host thread per rank, one
shared stream, the library's device-copy transport), on keys the equal slices
cannot spread: to_key(i) % 2^26, all of which land on shard 0.

Per group (P = 8, and P = 3 so cuts that are no power of two are covered):
  1. every rank inserts 5,000 distinct narrow keys with equal slices: shard 0
     holds everything (through the insert's overflow rounds), the others
     nothing;
  2. rebalance(): counts within 1 of N / P, every export inside its bounds,
     the same splitters on every rank and equal to the model's, check()
     passes, pages_used == bulk_plan(n).pages;
  3. routed gets (hits, 10 % misses, two batches in flight), routed inserts of
     new narrow keys plus deletes, and range scans spanning 1, 2 and P shards,
     against one unsharded oracle;
  4. a skewed second load, then rebalance() again: balanced again, contents
     unchanged;
  6. one rank with an arena too small for its share of a re-cut at one pair
     per leaf: every rank gets SHM_ENOMEM, and every tree's image and the
     splitters are unchanged;
  5. everything deleted but 3 pairs (repeated splitters, empty shards), then
     nothing (N = 0: the bounds stay): gets and scans still exact.
And at world 1 over RCCL with the routed path forced: rebalance is a
compaction, and gets after it are exact."""
import tempfile
import threading
import time
import traceback

import numpy as np
import pytest
import torch

from splitters_model import U64, equal_splitters, owner, rebalance_splitters
from test_multi_rank import free_port

pytestmark = pytest.mark.gpu

SPACE = 1 << 26
MAX_BATCH = 8192
PER_RANK = 5000
KEY_MAX = (1 << 64) - 1
SMALL = 1  # the rank with the small arena


def narrow_keys(first, n):
    from oracle.pyoracle import to_key
    return np.array([to_key(i) % SPACE for i in range(first, first + n)], dtype=U64)


_ALL = {}


def all_keys(P):
    """P * PER_RANK distinct narrow keys; rank r's are [r * PER_RANK, ...)"""
    if P not in _ALL:
        k = narrow_keys(1, P * PER_RANK + 200)
        _, idx = np.unique(k, return_index=True)
        _ALL[P] = k[np.sort(idx)][:P * PER_RANK]
    return _ALL[P]


def load1(r, P):
    k = all_keys(P)[r * PER_RANK:(r + 1) * PER_RANK]
    return k, k * U64(2) + U64(1)


def queries(seed, P):
    """4,000 gets: 90 % keys of load 1, 10 % never stored (the same n on every rank)"""
    rng = np.random.default_rng(300 + seed)
    pool = all_keys(P)
    q = pool[rng.integers(0, pool.size, 3600)]
    return np.concatenate([q, rng.integers(0, SPACE, 400, dtype=np.uint64) | U64(1 << 27)])


def load2(r, P):
    """new narrow keys (none of load 1's; a key two ranks share gets the same
    value from both) and deletes of some of this rank's load 1"""
    rng = np.random.default_rng(500 + r)
    k = np.setdiff1d(narrow_keys(10 ** 6 + 2000 * r, 1500), all_keys(P))
    mine, _ = load1(r, P)
    d = mine[10 + rng.integers(0, mine.size - 10, 300)]  # never the rank's first ten keys
    return np.concatenate([k, d]), np.concatenate([k + U64(7), np.zeros(d.size, dtype=U64)])


def load3(r, P):
    """skewed: 3,000 keys per rank that all sort above everything stored"""
    rng = np.random.default_rng(700 + r)
    k = np.unique(rng.integers(0, 1 << 20, 3000, dtype=np.uint64)) | U64(1 << 40) | U64(r << 21)
    return k, k ^ U64(0x5A5A)


def gets3(r, P):
    """the gets after load 2: its keys (new ones found, deleted ones missed)
    and the first batch again.  The same n on every rank: a routed get's slot
    size derives from n, and ranks that disagree exchange runs of different
    sizes (include/sherman_amd.h)"""
    return np.concatenate([np.resize(load2(r, P)[0], 1800), queries(r, P)])


def gets4(r, P):
    """the gets after load 3 (the same n on every rank, as gets3)"""
    return np.concatenate([np.resize(load3(r, P)[0], 3000), queries(r, P)])


def keep3(P):
    """the three pairs scenario 5 keeps: never deleted by load 2"""
    return np.sort(np.array([load1(r % P, P)[0][r] for r in range(3)], dtype=U64))


def scans(sp):
    """spans inside one shard, across each splitter (two shards), over all P,
    and an empty one"""
    lo = [1, 0, 5] + [max(s - 30000, 0) for s in sp]
    hi = [(sp[0] if sp else SPACE) // 2, KEY_MAX - 1, 4] + [s + 30000 for s in sp]
    return np.array(lo, dtype=U64), np.array(hi, dtype=U64)


SCANS5 = (np.array([0, 0, 7], dtype=U64), np.array([KEY_MAX - 1, SPACE, 6], dtype=U64))


def run_rank(r, P, trees, group, stream, out, errs):
    import sherman_amd as shm
    try:
        dev = torch.device("cuda:0")

        def d(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

        def routed_gets(cs, q):
            v = torch.empty(q.size, dtype=torch.int64, device=dev)
            f = torch.empty(q.size, dtype=torch.uint8, device=dev)
            cs.search(d(q), v, f, stream=stream)
            return v, f

        def routed_scans(cs, lo, hi):
            return cs.range_query(d(lo), d(hi), n_cap=64, stream=stream)

        def snap(cs, tree):
            """this rank's state after a step, for the main thread"""
            cs.synchronize()
            stream.synchronize()
            k, v = tree.export(stream=stream)
            return {"keys": k.cpu().numpy().view(U64), "vals": v.cpu().numpy().view(U64),
                    "sp": cs.splitters(), "pages": tree.stats()["pages_used"],
                    "check": tree.check()["keys"]}

        def delete_local(tree, keys):
            for o in range(0, keys.size, MAX_BATCH):
                part = keys[o:o + MAX_BATCH]
                tree.insert_batch(d(part), d(np.zeros(part.size, dtype=U64)), stream=stream)

        res = {}
        with torch.cuda.stream(stream):
            tree = trees[r]
            cs = shm.CShard.local(tree, group, r)
            res["sp0"] = cs.splitters()
            # 1. equal slices: everything lands on shard 0
            k, v = load1(r, P)
            cs.insert(d(k), d(v), stream=stream)
            res["s1"] = snap(cs, tree)
            # 2. rebalance
            res["n2"] = cs.rebalance(stream=stream)
            res["s2"] = snap(cs, tree)
            # 3. routed gets (two in flight), inserts + deletes, scans
            q1, q2 = queries(r, P), queries(r + 50, P)
            res["g1"] = routed_gets(cs, q1)
            a1, a2 = d(q1), d(q2)
            v1, f1 = torch.empty_like(a1), torch.empty(q1.size, dtype=torch.uint8, device=dev)
            v2, f2 = torch.empty_like(a2), torch.empty(q2.size, dtype=torch.uint8, device=dev)
            t1 = cs.search_begin(a1, stream=stream)
            t2 = cs.search_begin(a2, stream=stream)
            cs.search_end(t1, v1, f1)
            cs.search_end(t2, v2, f2)
            res["g1b"], res["g2b"] = (v1, f1), (v2, f2)
            k, v = load2(r, P)
            cs.insert(d(k), d(v), stream=stream)
            cs.synchronize()
            res["g3"] = routed_gets(cs, gets3(r, P))
            res["sc3"] = routed_scans(cs, *scans(res["s2"]["sp"]))
            res["s3"] = snap(cs, tree)
            # 4. a skewed load, rebalance again
            k, v = load3(r, P)
            cs.insert(d(k), d(v), stream=stream)
            res["s4a"] = snap(cs, tree)
            res["n4"] = cs.rebalance(stream=stream)
            res["s4"] = snap(cs, tree)
            res["g4"] = routed_gets(cs, gets4(r, P))
            res["sc4"] = routed_scans(cs, *scans(res["s4"]["sp"]))
            cs.synchronize()
            stream.synchronize()
            # 6. rank SMALL cannot hold its share at one pair per leaf
            before = (tree.dump_image()[0].tobytes(), cs.splitters())
            try:
                cs.rebalance(leaf_fill=1, stream=stream)
                res["rc6"] = 0
            except shm.ShermanError as e:
                res["rc6"] = e.rc
            res["same6"] = (tree.dump_image()[0].tobytes(), cs.splitters()) == before
            res["g6"] = routed_gets(cs, q1)
            # 5. all but three pairs deleted (each rank deletes what it stores), then all
            kept = keep3(P)
            delete_local(tree, np.setdiff1d(res["s4"]["keys"], kept))
            res["n5"] = cs.rebalance(stream=stream)
            res["s5"] = snap(cs, tree)
            q5 = np.concatenate([kept, q1[:1000]])
            res["g5"] = routed_gets(cs, q5)
            res["sc5"] = routed_scans(cs, *SCANS5)
            cs.synchronize()
            delete_local(tree, res["s5"]["keys"])
            res["n0"] = cs.rebalance(stream=stream)
            res["s0"] = snap(cs, tree)
            res["g0"] = routed_gets(cs, q5)
            res["sc0"] = routed_scans(cs, *SCANS5)
            cs.synchronize()
            stream.synchronize()
            for name, x in list(res.items()):
                if isinstance(x, tuple) and torch.is_tensor(x[0]):
                    res[name] = tuple(t.cpu().numpy() for t in x)
            cs.close()
        out[r] = res
    except BaseException as e:  # noqa: BLE001 - reported by the main thread
        # the other ranks now wait in a collective this rank never joins: the
        # main thread gives up on them (daemon threads) and reports this
        errs.append((r, repr(e), traceback.format_exc()))


def check_gets(ref, got, q, what):
    ov, of = ref.search_batch(q)
    assert np.array_equal(got[0].view(U64), ov), (what, int((got[0].view(U64) != ov).sum()))
    assert np.array_equal(got[1], of), what


def check_scans(ref, got, lo, hi, what):
    c, sv = got[0], got[1].view(U64)
    off = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    assert off[-1] == sv.size, what
    for i in range(lo.size):
        want, _ = ref.range_query(int(lo[i]), int(hi[i]))
        assert np.array_equal(np.sort(sv[off[i]:off[i + 1]]), np.sort(want)), (what, i)


def check_balanced(out, P, ref, nkey, skey, what):
    """after a rebalance: counts within 1 of N / P, exports inside the
    bounds, the model's splitters on every rank, compact trees, the
    unsharded contents"""
    import sherman_amd as shm
    rk, rv = ref.dump()
    o = np.argsort(rk)
    rk, rv = rk[o], rv[o]
    N = rk.size
    want_sp = rebalance_splitters(rk, P)
    ks, vs = [], []
    for r in range(P):
        s, n = out[r][skey], out[r][nkey]
        assert abs(n - N / P) < 1, (what, r, n, N)
        assert s["keys"].size == n == s["check"], (what, r)
        assert s["sp"] == want_sp, (what, r)
        assert bool((owner(s["keys"], s["sp"]) == r).all()), (what, r)
        assert np.all(s["keys"][1:] > s["keys"][:-1])
        assert s["pages"] == shm.bulk_plan(n)["pages"], (what, r, s["pages"])
        ks.append(s["keys"])
        vs.append(s["vals"])
    # rank order is key order: the concatenation is the global sorted run
    assert np.array_equal(np.concatenate(ks), rk) and np.array_equal(np.concatenate(vs), rv), what
    return want_sp


@pytest.mark.parametrize("P", [8, 3])
def test_rebalance_in_the_local_group(P):
    import sherman_amd as shm
    from oracle.pyoracle import OracleTree
    from sherman_amd.shard import shard_range

    assert torch.cuda.is_available(), "GPU test without a GPU"
    torch.cuda.set_device(0)
    trees = []
    for r in range(P):
        lo, bits = shard_range(r, P)
        trees.append(shm.Tree(arena_bytes=(6 << 20) if r == SMALL else (32 << 20),
                              max_batch=MAX_BATCH, device=0, node_id=r, key_lo=lo, key_bits=bits))
    group = shm.LocalGroup(P)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    out, errs = [None] * P, []
    th = [threading.Thread(target=run_rank, args=(r, P, trees, group, stream, out, errs),
                           daemon=True) for r in range(P)]
    for t in th:
        t.start()
    deadline = time.monotonic() + 120
    for t in th:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    assert not errs, errs
    assert not any(t.is_alive() for t in th), "a rank thread hung"
    torch.cuda.synchronize()

    ref = OracleTree(64 << 20)
    for r in range(P):
        ref.apply_batch(*load1(r, P))
    # 1. equal slices put every narrow key on shard 0
    eq = equal_splitters(P)
    for r in range(P):
        assert out[r]["sp0"] == eq and out[r]["s1"]["sp"] == eq
        assert out[r]["s1"]["keys"].size == (P * PER_RANK if r == 0 else 0), r
    # 2.
    sp2 = check_balanced(out, P, ref, "n2", "s2", "first rebalance")
    assert all(out[r]["n2"] == PER_RANK for r in range(P))
    assert sp2 != eq and sp2[-1] < SPACE
    # 3.
    for r in range(P):
        check_gets(ref, out[r]["g1"], queries(r, P), ("g1", r))
        check_gets(ref, out[r]["g1b"], queries(r, P), ("g1b", r))
        check_gets(ref, out[r]["g2b"], queries(r + 50, P), ("g2b", r))
    for r in range(P):
        ref.apply_batch(*load2(r, P))
    for r in range(P):
        check_gets(ref, out[r]["g3"], gets3(r, P), ("g3", r))
        check_scans(ref, out[r]["sc3"], *scans(sp2), ("sc3", r))
        s = out[r]["s3"]
        assert s["sp"] == sp2 and bool((owner(s["keys"], sp2) == r).all()), r
    rk, _ = ref.dump()
    assert sum(out[r]["s3"]["keys"].size for r in range(P)) == rk.size
    # 4. the skewed load lands on the last shard; the second rebalance evens it out
    for r in range(P):
        ref.apply_batch(*load3(r, P))
    sizes = [out[r]["s4a"]["keys"].size for r in range(P)]
    assert sizes[P - 1] > 2 * max(sizes[:P - 1]), sizes
    sp4 = check_balanced(out, P, ref, "n4", "s4", "second rebalance")
    for r in range(P):
        check_gets(ref, out[r]["g4"], gets4(r, P), ("g4", r))
        check_scans(ref, out[r]["sc4"], *scans(sp4), ("sc4", r))
    # 6. every rank refused, nothing changed
    for r in range(P):
        assert out[r]["rc6"] == shm.SHM_ENOMEM, (r, out[r]["rc6"])
        assert out[r]["same6"], r
        check_gets(ref, out[r]["g6"], queries(r, P), ("g6", r))
    # 5. three pairs: repeated splitters, empty shards
    kept = keep3(P)
    rk, _ = ref.dump()
    gone = np.setdiff1d(rk, kept)
    ref.apply_batch(gone, np.zeros(gone.size, dtype=U64))
    sp5 = check_balanced(out, P, ref, "n5", "s5", "three pairs")
    assert sum(out[r]["n5"] for r in range(P)) == 3
    if P > 3:
        assert len(set(sp5)) < len(sp5)  # cuts coincide
    for r in range(P):
        check_gets(ref, out[r]["g5"], np.concatenate([kept, queries(r, P)[:1000]]), ("g5", r))
        check_scans(ref, out[r]["sc5"], *SCANS5, ("sc5", r))
    # N = 0: nothing loaded, the bounds stay
    ref.apply_batch(kept, np.zeros(3, dtype=U64))
    for r in range(P):
        assert out[r]["n0"] == 0 and out[r]["s0"]["keys"].size == 0
        assert out[r]["s0"]["sp"] == sp5
        check_gets(ref, out[r]["g0"], np.concatenate([kept, queries(r, P)[:1000]]), ("g0", r))
        check_scans(ref, out[r]["sc0"], *SCANS5, ("sc0", r))
    ref.close()
    group.close()
    for t in trees:
        t.close()


def world1_worker(rank, port, outdir):
    import torch.distributed as dist

    import sherman_amd as shm
    from oracle.pyoracle import OracleTree

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=dev)

    def d(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    tree = shm.Tree(arena_bytes=32 << 20, max_batch=MAX_BATCH, device=0)
    cs = shm.CShard(tree, 1, 0, dist)
    cs.force_route(True)
    ref = OracleTree(64 << 20)
    k, v = load1(0, 1)
    cs.insert(d(k), d(v))
    ref.apply_batch(k, v)
    gone = k[::3]
    cs.insert(d(gone), d(np.zeros(gone.size, dtype=U64)))
    ref.apply_batch(gone, np.zeros(gone.size, dtype=U64))
    cs.synchronize()
    pages_before = tree.stats()["pages_used"]
    n = cs.rebalance()
    rk, rv = ref.dump()
    assert n == rk.size == tree.check()["keys"]
    assert cs.splitters() == []
    assert tree.stats()["pages_used"] == shm.bulk_plan(n)["pages"] < pages_before
    q = queries(0, 1)
    vals = torch.empty(q.size, dtype=torch.int64, device=dev)
    found = torch.empty(q.size, dtype=torch.uint8, device=dev)
    cs.search(d(q), vals, found)
    cs.synchronize()
    check_gets(ref, (vals.cpu().numpy(), found.cpu().numpy()), q, "world 1")
    ek, ev = tree.export()
    o = np.argsort(rk)
    assert np.array_equal(ek.cpu().numpy().view(U64), rk[o])
    assert np.array_equal(ev.cpu().numpy().view(U64), rv[o])
    # the hint follows the run: its first key, the bits of its span
    _, info = tree.dir_dump()
    span = int(rk.max() - rk.min()) + 1
    assert info["lo"] == int(rk.min())
    assert info["shift"] + tree.dir_stats()["bits"] == max(1, (span - 1).bit_length())
    ref.close()
    cs.close()
    tree.close()
    dist.destroy_process_group()


def test_rebalance_at_world_1_over_rccl_is_a_compaction():
    import torch.multiprocessing as mp
    assert torch.cuda.is_available(), "GPU test without a GPU"
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(world1_worker, args=(free_port(), d), nprocs=1, join=True)


def splitters_rank(r, P, trees, group, stream, sp, out, errs):
    import sherman_amd as shm
    try:
        dev = torch.device("cuda:0")

        def d(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

        res = {}
        with torch.cuda.stream(stream):
            tree = trees[r]
            cs = shm.CShard.local(tree, group, r)
            # ranks that disagree: every rank is refused and keeps its bounds
            try:
                cs.set_splitters([x + (1 if r == 1 else 0) for x in sp])
                res["rc_diff"] = 0
            except shm.ShermanError as e:
                res["rc_diff"] = e.rc
            res["sp_after_diff"] = cs.splitters()
            try:
                cs.set_splitters(sp[::-1])
                res["rc_desc"] = 0
            except shm.ShermanError as e:
                res["rc_desc"] = e.rc
            cs.set_splitters(sp)
            res["sp"] = cs.splitters()
            k, v = load1(r, P)
            cs.insert(d(k), d(v), stream=stream)
            cs.synchronize()
            q = queries(r, P)
            vals = torch.empty(q.size, dtype=torch.int64, device=dev)
            found = torch.empty(q.size, dtype=torch.uint8, device=dev)
            cs.search(d(q), vals, found, stream=stream)
            res["sc"] = cs.range_query(d(np.array([0, sp[0] - 1000], dtype=U64)),
                                       d(np.array([KEY_MAX - 1, sp[0] + 1000], dtype=U64)),
                                       n_cap=64, stream=stream)
            cs.synchronize()
            stream.synchronize()
            ek, _ = tree.export(stream=stream)
            res["keys"] = ek.cpu().numpy().view(U64)
            res["g"] = (vals.cpu().numpy(), found.cpu().numpy())
            res["sc"] = tuple(t.cpu().numpy() for t in res["sc"])
            cs.set_splitters(None)
            res["sp_none"] = cs.splitters()
            cs.close()
        out[r] = res
    except BaseException as e:  # noqa: BLE001 - reported by the main thread
        errs.append((r, repr(e), traceback.format_exc()))


def test_set_splitters_on_empty_trees_in_the_local_group():
    """P = 3: splitters chosen by the caller before the first load (the
    model's quantiles of the keys to come).  Ranks that pass different words,
    or descending ones, get SHM_EINVAL and keep their bounds; with the
    splitters set, routed inserts spread the narrow keys evenly, every shard
    holds only keys inside its bounds, gets and scans are exact; NULL returns
    to the equal slices."""
    import sherman_amd as shm
    from oracle.pyoracle import OracleTree

    assert torch.cuda.is_available(), "GPU test without a GPU"
    torch.cuda.set_device(0)
    P = 3
    sp = rebalance_splitters(np.sort(all_keys(P)), P)
    trees = [shm.Tree(arena_bytes=32 << 20, max_batch=MAX_BATCH, device=0, node_id=r)
             for r in range(P)]
    group = shm.LocalGroup(P)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    out, errs = [None] * P, []
    th = [threading.Thread(target=splitters_rank, args=(r, P, trees, group, stream, sp, out, errs),
                           daemon=True) for r in range(P)]
    for t in th:
        t.start()
    deadline = time.monotonic() + 120
    for t in th:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    assert not errs, errs
    assert not any(t.is_alive() for t in th), "a rank thread hung"
    ref = OracleTree(64 << 20)
    for r in range(P):
        ref.apply_batch(*load1(r, P))
    eq = equal_splitters(P)
    for r in range(P):
        x = out[r]
        assert x["rc_diff"] == shm.SHM_EINVAL and x["sp_after_diff"] == eq
        assert x["rc_desc"] == shm.SHM_EINVAL
        assert x["sp"] == sp and x["sp_none"] == eq
        assert x["keys"].size == PER_RANK and bool((owner(x["keys"], sp) == r).all())
        check_gets(ref, x["g"], queries(r, P), ("set_splitters", r))
        check_scans(ref, x["sc"], np.array([0, sp[0] - 1000], dtype=U64),
                    np.array([KEY_MAX - 1, sp[0] + 1000], dtype=U64), ("set_splitters", r))
    ref.close()
    group.close()
    for t in trees:
        t.close()
