"""Host model of splitter routing and of the rebalance plan (numpy / Python
ints only): what route.hip's owner search, shm_route_bucket_bounds and
shm_rebalance_plan must compute.

Owner rule: shard p owns [b[p], b[p + 1]) with b[0] = 0, b[P] = 2^64 and
b[1 .. P - 1] the splitters (ascending, repeats allowed), so a key's owner is
the number of splitters <= it: numpy.searchsorted(side="right").  A repeated
splitter x leaves the shards between its first and last copy empty, and a key
equal to x goes to the highest shard that starts at x.

Plan: shards are range-ordered, so the global sorted order is the shards'
sorted contents in rank order.  With N = sum(counts) and off the exclusive
scan, old shard r holds global positions [off[r], off[r] + counts[r]); new
shard p holds [cut[p], cut[p + 1]) with cut[p] = floor(p N / P).
"""
import numpy as np

U64 = np.uint64
KEY_MAX = (1 << 64) - 1


def equal_splitters(P):
    """the equal slices' boundaries ceil(p 2^64 / P), p = 1 .. P - 1"""
    return [((p << 64) + P - 1) // P for p in range(1, P)]


def owner(keys, splitters):
    """owner of each u64 key: the number of splitters <= it"""
    sp = np.asarray(splitters, dtype=U64)
    return np.searchsorted(sp, np.asarray(keys, dtype=U64), side="right").astype(np.int64)


def bucket(keys, P, splitters):
    """shm_route_bucket_bounds: (counts[P], keys grouped by owner keeping the
    input order inside a shard, perm[i] = input position of keys_out[i])"""
    keys = np.asarray(keys, dtype=U64)
    own = owner(keys, splitters)
    perm = np.argsort(own, kind="stable")
    return np.bincount(own, minlength=P).astype(np.uint64), keys[perm], perm.astype(np.uint32)


def overlap(a0, a1, b0, b1):
    return max(0, min(a1, b1) - max(a0, b0))


def rebalance_plan(counts, rank):
    """(cut[P + 1], send_cnt[P], recv_cnt[P]) of `rank`, in Python ints"""
    P = len(counts)
    off = [0]
    for c in counts:
        off.append(off[-1] + int(c))
    N = off[P]
    cut = [p * N // P for p in range(P + 1)]
    send = [overlap(off[rank], off[rank + 1], cut[p], cut[p + 1]) for p in range(P)]
    recv = [overlap(off[p], off[p + 1], cut[rank], cut[rank + 1]) for p in range(P)]
    return cut, send, recv


def rebalance_splitters(sorted_keys, P):
    """the splitters a rebalance installs for the global ascending run
    sorted_keys: splitter j = the key at position cut[j] (N > 0)"""
    N = len(sorted_keys)
    return [int(sorted_keys[j * N // P]) for j in range(1, P)]
