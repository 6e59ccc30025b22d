"""Wall time of CShard.rebalance() for 8 x 2^20 pairs in the in-process group
on one GPU (eight trees, one host thread per rank, one shared stream, device
copies for the exchange) beside Tree.compact() of one tree holding the same
2^23 pairs: the same export and bulk-load passes, plus the count and splitter
exchanges, the move and eight trees' worth of host calls.  The keys are
skewed (u^2 over the key space), so the equal slices hold 35 % .. 6.5 % of
them and most pairs move.  A first number for later work, not a rate the
multi-GPU path can be held to: the real exchange is RCCL over xGMI.
usage: python tools/rebalance_rate.py [pairs_log2] [P]"""
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sherman_amd as shm
from sherman_amd.shard import owner_of

kl = int(sys.argv[1]) if len(sys.argv) > 1 else 23
P = int(sys.argv[2]) if len(sys.argv) > 2 else 8
torch.cuda.set_device(0)
dev = torch.device("cuda:0")
n = 1 << kl
rng = np.random.default_rng(1)
u = rng.random(n + n // 64)
keys = np.unique((u * u * float(1 << 63)).astype(np.uint64) * np.uint64(2) + np.uint64(1))[:n]
n = keys.size
vals = keys ^ np.uint64(0x1234567)
own = owner_of(torch.from_numpy(keys.view(np.int64)), P).numpy()
arena = max(64 << 20, n * 64)


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)


trees, before = [], []
for r in range(P):
    t = shm.Tree(arena_bytes=arena, max_batch=8192, device=0, node_id=r)
    m = own == r
    t.bulk_load(d(keys[m]), d(vals[m]))
    before.append(int(m.sum()))
    trees.append(t)
group = shm.LocalGroup(P)
stream = torch.cuda.Stream()
stream.wait_stream(torch.cuda.current_stream())
torch.cuda.synchronize()
gate = threading.Barrier(P + 1)
after, errs, t_end = [0] * P, [], [0.0] * P


def rank(r):
    try:
        with torch.cuda.stream(stream):
            cs = shm.CShard.local(trees[r], group, r)
            gate.wait()
            after[r] = cs.rebalance(stream=stream)
            t_end[r] = time.perf_counter()
            gate.wait()
            cs.close()
    except BaseException as e:  # noqa: BLE001
        errs.append((r, repr(e)))
        gate.abort()


th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
for x in th:
    x.start()
gate.wait()
t0 = time.perf_counter()
gate.wait()
for x in th:
    x.join()
assert not errs, errs
reb_ms = (max(t_end) - t0) * 1e3
assert sum(after) == n and max(after) - min(after) <= 1
group.close()
for t in trees:
    t.close()

one = shm.Tree(arena_bytes=arena * 2, max_batch=8192, device=0)
one.bulk_load(d(keys), d(vals))
torch.cuda.synchronize()
c = []
for _ in range(3):
    t0 = time.perf_counter()
    one.compact()
    c.append((time.perf_counter() - t0) * 1e3)
one.close()
print(json.dumps({"pairs": n, "P": P, "pairs_per_rank_before": before,
                  "pairs_per_rank_after": after, "rebalance_ms": round(reb_ms, 2),
                  "rebalance_mpairs_per_s": round(n / reb_ms / 1e3, 1),
                  "compact_one_tree_ms": [round(x, 2) for x in c],
                  "condition": "in-process group on one GPU (device copies, no RCCL), wall "
                               "clock from the ranks' common start to the last rank's return; "
                               "compact() of one tree holding all the pairs, three calls"}))
