"""The splitter model's own properties, shm_rebalance_plan (through ctypes: it
is host arithmetic and needs no GPU) against the model, and shard.py's
owner_of(..., splitters) against numpy.searchsorted(side="right")."""
import ctypes

import numpy as np
import pytest
import torch

import sherman_amd as shm
from sherman_amd.shard import owner_of, shard_bounds
from splitters_model import (KEY_MAX, U64, bucket, equal_splitters, owner, rebalance_plan,
                             rebalance_splitters)

WORLDS = [1, 2, 3, 8, 16]


def count_cases(P):
    rng = np.random.default_rng(17 + P)
    cases = [[0] * P,                                   # N = 0
             [1] + [0] * (P - 1),                       # N < P (P > 1)
             [0] * (P - 1) + [max(P - 1, 1)],           # N < P, all on the last rank
             [40000] + [0] * (P - 1),                   # all pairs on one rank
             [0] * (P - 1) + [12345],
             [7] * P,
             [int(x) for x in rng.integers(0, 5000, P)],
             [int(x) for x in rng.integers(0, 3, P)],
             [(1 << 40) + 3] * P]                       # products past 2^32
    return cases


@pytest.mark.parametrize("P", WORLDS)
def test_plan_properties(P):
    for counts in count_cases(P):
        N = sum(counts)
        plans = [rebalance_plan(counts, r) for r in range(P)]
        new = []
        for r, (cut, send, recv) in enumerate(plans):
            assert cut[0] == 0 and cut[P] == N and cut == sorted(cut)
            assert sum(send) == counts[r]
            assert sum(recv) == cut[r + 1] - cut[r]
            new.append(sum(recv))
        assert sum(new) == N and max(new) - min(new) <= 1
        for a in range(P):
            for b in range(P):
                assert plans[a][1][b] == plans[b][2][a]  # a sends b what b receives from a


@pytest.mark.parametrize("P", WORLDS)
def test_c_plan_equals_model(P):
    L = shm.lib()
    for counts in count_cases(P):
        for r in range(P):
            got = shm.rebalance_plan(counts, r)
            cut, send, recv = rebalance_plan(counts, r)
            assert got == {"cut": cut, "send": send, "recv": recv}, (counts, r)
    c = (ctypes.c_uint64 * 17)()
    o = (ctypes.c_uint64 * 18)()
    for P_bad, rank in ((0, 0), (17, 0), (P, P), (P, P + 5)):
        assert L.shm_rebalance_plan(c, P_bad, rank, o, o, o) == shm.SHM_EINVAL
    assert L.shm_rebalance_plan(None, P, 0, o, o, o) == shm.SHM_EINVAL
    assert L.shm_rebalance_plan(c, P, 0, None, o, o) == shm.SHM_EINVAL
    assert all(x == 0 for x in o)


def test_rebalance_splitters_route_every_key_to_its_new_shard():
    """splitter j = the key at position cut[j]: with the owner rule, position
    i of the global run lands on the shard whose [cut[p], cut[p + 1]) holds it,
    also when cuts coincide (N < P: repeated splitters, empty shards)."""
    rng = np.random.default_rng(5)
    for P in WORLDS:
        for N in (1, 2, 3, P, P + 1, 1000):
            keys = np.unique(rng.integers(0, 1 << 26, 4 * N, dtype=np.uint64))[:N]
            N = keys.size
            sp = rebalance_splitters(keys, P)
            assert sp == sorted(sp)
            own = owner(keys, sp)
            cut = [p * N // P for p in range(P + 1)]
            want = np.searchsorted(np.array(cut[1:], dtype=np.int64), np.arange(N), side="right")
            assert np.array_equal(own, want), (P, N)


def edge_keys(splitters):
    ks = {0, 1, KEY_MAX - 1}
    for s in splitters:
        ks.update(x for x in (s - 1, s, s + 1) if 0 <= x < KEY_MAX)
    return np.array(sorted(ks), dtype=U64)


SPLIT_CASES = [
    (1, []),
    (2, [1 << 25]),
    (3, [5, 5]),                                   # a repeated splitter: shard 1 = [5, 5)
    (4, [0, 0, 7]),                                # shards 0 and 1 empty (b = 0)
    (8, [10, 20, 20, 20, 1 << 26, 1 << 63, (1 << 63) + 1]),  # three equal; across the sign bit
    (8, equal_splitters(8)),
    (16, [KEY_MAX - 1] * 15),                      # everything below goes to shard 0
]


@pytest.mark.parametrize("P,sp", SPLIT_CASES)
def test_torch_owner_of_equals_searchsorted_right(P, sp):
    rng = np.random.default_rng(P)
    keys = np.concatenate([edge_keys(sp), rng.integers(0, KEY_MAX, 500, dtype=np.uint64),
                           rng.integers(0, 1 << 27, 500, dtype=np.uint64)])
    t = torch.from_numpy(keys.view(np.int64))
    got = owner_of(t, P, sp).numpy()
    assert np.array_equal(got, owner(keys, sp))
    # numpy u64 and int64-tensor splitters are the same splitters
    assert np.array_equal(owner_of(t, P, np.array(sp, dtype=U64)).numpy(), got)
    b = shard_bounds(P, "cpu", sp).numpy().view(U64)
    assert b[0] == 0 and b[P] == KEY_MAX and [int(x) for x in b[1:P]] == sp


def test_equal_splitters_give_the_equal_slices():
    rng = np.random.default_rng(3)
    keys = rng.integers(0, KEY_MAX, 4000, dtype=np.uint64)
    t = torch.from_numpy(keys.view(np.int64))
    for P in (2, 3, 8, 16):
        sp = equal_splitters(P)
        assert np.array_equal(owner_of(t, P, sp).numpy(), owner_of(t, P).numpy())
        assert torch.equal(shard_bounds(P, "cpu", sp), shard_bounds(P, "cpu"))


def test_bucket_model_is_stable_and_a_permutation():
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 100, 1000, dtype=np.uint64)
    counts, ko, perm = bucket(keys, 4, [10, 10, 60])
    assert counts.tolist() == [int((keys < 10).sum()), 0, int(((keys >= 10) & (keys < 60)).sum()),
                               int((keys >= 60).sum())]
    assert np.array_equal(ko, keys[perm]) and sorted(perm.tolist()) == list(range(1000))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    for p in range(4):
        assert np.all(np.diff(perm[off[p]:off[p + 1]].astype(np.int64)) > 0)


def test_descending_or_keymax_splitters_are_refused():
    t = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError):
        owner_of(t, 3, [9, 8])
    with pytest.raises(ValueError):
        owner_of(t, 3, [9, KEY_MAX])
    with pytest.raises(ValueError):
        owner_of(t, 3, [9])
