"""ShardRouter(splitters=...) over gloo at world 2 and 3, on keys that equal
slices cannot spread: to_key(i) % 2^26 (the reference's benchmark key set),
every one of which the equal slices give to shard 0.

The splitters come from sample_splitters over each rank's first batch.
Checked against ONE unsharded oracle tree: the union of the shards after
routed inserts (with deletes and cross-rank conflicts), every shard holding
only keys inside its bounds, shard sizes within 12.5 % of N / P, routed gets
with misses, and range scans that cross a splitter (also with a repeated
splitter, i.e. an empty shard in the middle).
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.pyoracle import OracleTree, to_key
from sherman_amd.shard import ShardRouter, owner_of, sample_splitters
from splitters_model import owner
from test_multi_rank import OracleShard, free_port

U64 = np.uint64
SPACE = 1 << 26
N_KEYS = 3000


def c1_keys():
    return np.array([to_key(i) % SPACE for i in range(1, N_KEYS + 1)], dtype=U64)


class SplitOracleShard(OracleShard):
    def route_bucket(self, keys, world, keys_out, perm_out, counts_out, splitters=None):
        own = owner_of(keys, world, splitters)
        order = torch.argsort(own, stable=True)
        keys_out.copy_(keys[order])
        perm_out.copy_(order.to(torch.int32))
        counts_out.copy_(torch.bincount(own, minlength=world))


def rank_rounds(rank, world):
    """Round 0: the rank's stride of the key set (what it samples); round 1:
    keys from the whole set again (cross-rank conflicts), 5 % deletes."""
    keys = c1_keys()
    rng = np.random.default_rng(40 + rank)
    k0 = keys[rank::world]
    v0 = np.arange(k0.size, dtype=U64) + U64(1 + 10 ** 6 * rank)
    k1 = keys[rng.integers(0, keys.size, 1500)]
    v1 = np.arange(1500, dtype=U64) + U64(5 * 10 ** 7 + 10 ** 6 * rank)
    v1[rng.random(1500) < 0.05] = 0
    return [(k0, v0), (k1, v1)]


def rank_queries(rank):
    rng = np.random.default_rng(60 + rank)
    ids = rng.integers(1, 2 * N_KEYS, 4000)  # about half never inserted
    return np.array([to_key(int(i)) % SPACE for i in ids], dtype=U64)


def rank_scans(rank, sp):
    """Scans around every splitter (crossing it), over everything, empty,
    from a splitter to the top, and narrow random ones."""
    rng = np.random.default_rng(80 + rank)
    lo, hi = [], []
    for s in sp:
        lo += [max(s - SPACE // 16, 0), s, s - 1, 0]
        hi += [s + SPACE // 16, s, s, s]
    lo += [0, 0, 5, sp[0]]
    hi += [(1 << 64) - 1, SPACE, 4, (1 << 64) - 2]
    a = rng.integers(0, SPACE, 20)
    lo += a.tolist()
    hi += (a + rng.integers(0, SPACE // 8, 20)).tolist()
    return np.array(lo, dtype=U64), np.array(hi, dtype=U64)


def worker(rank, world, port, outdir, fixed):
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}",
                            rank=rank, world_size=world)

    def t64(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))

    rounds = rank_rounds(rank, world)
    sp = fixed if fixed is not None else sample_splitters(t64(rounds[0][0]), world, dist)
    shard = SplitOracleShard()
    router = ShardRouter(shard, world, dist, splitters=sp)
    for k, v in rounds:
        router.insert(t64(k), t64(v))
    q = rank_queries(rank)
    vals = torch.empty(q.size, dtype=torch.int64)
    found = torch.empty(q.size, dtype=torch.uint8)
    router.search(t64(q), vals, found)
    slo, shi = rank_scans(rank, sp)
    counts, svals = router.range_query(t64(slo), t64(shi))
    keys, values = shard.t.dump()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), keys=keys, values=values,
             vals=vals.numpy(), found=found.numpy(), sp=np.array(sp, dtype=U64),
             scounts=counts.numpy(), svals=svals.numpy())
    shard.t.close()
    dist.barrier()
    dist.destroy_process_group()


def verify(d, world, balanced):
    res = [np.load(os.path.join(d, f"rank{r}.npz")) for r in range(world)]
    sp = [int(x) for x in res[0]["sp"]]
    for x in res:
        assert [int(v) for v in x["sp"]] == sp  # the same splitters on every rank
    ref = OracleTree(64 << 20)
    for rnd in range(2):
        for r in range(world):
            ref.apply_batch(*rank_rounds(r, world)[rnd])
    rk, rv = ref.dump()
    o = np.argsort(rk)
    rk, rv = rk[o], rv[o]
    uk = np.concatenate([x["keys"] for x in res])
    uv = np.concatenate([x["values"] for x in res])
    o = np.argsort(uk)
    assert np.array_equal(uk[o], rk) and np.array_equal(uv[o], rv)
    key_of = dict(zip(rv.tolist(), rk.tolist()))
    for r, x in enumerate(res):
        assert bool((owner(x["keys"], sp) == r).all())  # only keys inside its bounds
        if balanced:
            # the sample alone meets the bound: each shard within 12.5 % of N / P
            assert abs(x["keys"].size - rk.size / world) <= 0.125 * rk.size / world, \
                (r, x["keys"].size, rk.size)
        ov, of = ref.search_batch(rank_queries(r))
        assert np.array_equal(x["vals"].view(U64), ov) and np.array_equal(x["found"], of)
        assert 0.2 < of.mean() < 0.8  # hits and misses
        slo, shi = rank_scans(r, sp)
        off = np.concatenate([[0], np.cumsum(x["scounts"])])
        assert off[-1] == x["svals"].size
        crossing = 0
        for i in range(slo.size):
            want, _ = ref.range_query(int(slo[i]), int(shi[i]))
            got = x["svals"][off[i]:off[i + 1]].view(U64)
            assert np.array_equal(np.sort(got), np.sort(want)), (r, i)
            own = owner(np.array([key_of[v] for v in got.tolist()], dtype=U64), sp)
            assert bool((own[1:] >= own[:-1]).all()), (r, i)  # shard order = key order
            crossing += own.size > 0 and own[0] != own[-1]
        assert crossing >= len(sp)
    # the equal slices would have put every key on shard 0
    assert bool((owner_of(torch.from_numpy(rk.view(np.int64)), world) == 0).all())
    ref.close()


@pytest.mark.parametrize("world", [2, 3])
def test_sampled_splitters_spread_narrow_keys_and_route_exactly(world):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(worker, args=(world, free_port(), d, None), nprocs=world, join=True)
        verify(d, world, balanced=True)


def test_a_repeated_splitter_leaves_an_empty_shard_between_two_others():
    """world 3, splitters [x, x]: shard 1 = [x, x) holds nothing, a key equal
    to x belongs to shard 2, and scans across x skip the empty shard."""
    x = int(np.sort(c1_keys())[N_KEYS // 2])  # a stored key
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(worker, args=(3, free_port(), d, [x, x]), nprocs=3, join=True)
        verify(d, 3, balanced=False)
        assert np.load(os.path.join(d, "rank1.npz"))["keys"].size == 0
        assert x in np.load(os.path.join(d, "rank2.npz"))["keys"].tolist()
