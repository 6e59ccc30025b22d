"""Routing by splitters on the GPU against the numpy model
(tests/splitters_model.py): shm_route_bucket_bounds' counts, stable order and
perm, in both forms of the owner search (splitters in the kernel arguments /
binary search in LDS), the routed get's slot placement with bounds
(shm__route_slots_bounds), the kKeyMax rejection of a routed insert's
bucketing, and splitters=None equal to shm_route_bucket bit for bit.

Sizes sit on either side of the 1024-key tile of k_route_count /
k_route_scatter and of the 4096-key block k_route_slots places, and 8191 at
max_batch 8192 covers the second block's edge."""
import ctypes

import numpy as np
import pytest
import torch

from splitters_model import KEY_MAX, U64, bucket, equal_splitters, owner

pytestmark = pytest.mark.gpu

MAX_BATCH = 8192
SIZES = [1, 1023, 1024, 1025, 4095, 4097, 8191]
BIG = 10000  # its own tree: past MAX_BATCH


def splitters_for(P, kind):
    rng = np.random.default_rng(1000 + P)
    if P == 1:
        return []
    if kind == "narrow":  # cuts of [0, 2^26): what a rebalance of narrow keys installs
        return sorted(int(x) for x in rng.integers(1, 1 << 26, P - 1))
    if kind == "wide":    # across the sign bit and near the top
        sp = sorted(int(x) for x in rng.integers(0, KEY_MAX, P - 1, dtype=np.uint64))
        sp[-1] = KEY_MAX - 1
        return sp
    if kind == "equal3":  # three equal splitters (P >= 4): two empty shards
        sp = sorted(int(x) for x in rng.integers(1, 1 << 26, P - 1))
        m = (P - 1) // 2
        sp[m - 1] = sp[m + 1] = sp[m]
        return sp
    if kind == "one":     # every key in one shard: all splitters above the keys
        return [(1 << 40) + j for j in range(P - 1)]
    if kind == "zero":    # splitters at 0: the first shards own nothing
        return [0] * ((P - 1) // 2) + [1 << 25] * (P - 1 - (P - 1) // 2)
    raise AssertionError(kind)


def keys_for(n, sp, seed):
    """n keys: every splitter, splitter +- 1, 0 and 2^64 - 2 first, then keys
    below 2^26 and over the whole space, shuffled"""
    rng = np.random.default_rng(seed)
    edge = {0, KEY_MAX - 1}
    for s in sp:
        edge.update(x for x in (s - 1, s, s + 1) if 0 <= x < KEY_MAX)
    edge = np.array(sorted(edge), dtype=U64)
    rest = np.concatenate([rng.integers(0, 1 << 26, n, dtype=np.uint64),
                           rng.integers(0, KEY_MAX, n // 4 + 1, dtype=np.uint64)])
    rng.shuffle(rest)
    k = np.concatenate([edge, rest])[:n]
    rng.shuffle(k)
    return k


@pytest.fixture(scope="module")
def tree():
    import sherman_amd as shm
    assert torch.cuda.is_available(), "GPU test without a GPU"
    torch.cuda.set_device(0)
    t = shm.Tree(arena_bytes=16 << 20, max_batch=MAX_BATCH)
    yield t
    t.close()


@pytest.fixture(scope="module")
def hooks():
    import sherman_amd as shm
    L = shm.lib()
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.shm__route_bucket_mode.restype = ctypes.c_int
    L.shm__route_bucket_mode.argtypes = [vp, vp, u64, u32, vp, ctypes.c_int, vp, vp, vp, vp]
    L.shm__route_slots_bounds.restype = ctypes.c_int
    L.shm__route_slots_bounds.argtypes = [vp, vp, u64, u32, u64, vp, vp, vp, vp, vp, ctypes.c_int,
                                          vp, ctypes.c_int, vp]
    L.shm__route_bucket_insert.restype = ctypes.c_int
    L.shm__route_bucket_insert.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp, vp]
    return L


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def run_bucket(t, L, keys, P, sp, mode):
    n = keys.size
    kd = dev64(keys)
    ko = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    perm = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((P,), -1, dtype=torch.int64, device="cuda")
    if mode is None:
        t.route_bucket(kd, P, ko, perm, cnt, splitters=sp)
    else:
        arr = (ctypes.c_uint64 * max(len(sp), 1))(*sp)
        assert L.shm__route_bucket_mode(t.h, kd.data_ptr(), n, P, arr, mode, cnt.data_ptr(),
                                        ko.data_ptr(), perm.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return (cnt.cpu().numpy().view(U64), ko.cpu().numpy().view(U64),
            perm.cpu().numpy().view(np.uint32))


def check_bucket(got, keys, P, sp):
    c, ko, perm = bucket(keys, P, sp)
    assert np.array_equal(got[0], c)
    assert np.array_equal(got[2], perm)   # stable: the model's argsort is the only answer
    assert np.array_equal(got[1], ko)


CASES = [(1, "narrow"), (2, "narrow"), (3, "narrow"), (3, "wide"), (8, "narrow"), (8, "equal3"),
         (8, "one"), (8, "zero"), (8, "wide"), (16, "narrow"), (64, "narrow"), (64, "equal3"),
         (64, "wide")]


@pytest.mark.parametrize("P,kind", CASES)
def test_bucket_with_splitters_equals_the_model(tree, hooks, P, kind):
    sp = splitters_for(P, kind)
    for n in SIZES:
        keys = keys_for(n, sp, 7 * n + P)
        # the form the library picks, then each form by name (the kernel
        # arguments serve P <= 16 only; past that the hook takes the LDS form)
        for mode in (None, 1, 2):
            check_bucket(run_bucket(tree, hooks, keys, P, sp, mode), keys, P, sp)
    if kind == "one":
        got = run_bucket(tree, hooks, keys_for(4097, sp, 3) % U64(1 << 26), P, sp, None)
        assert got[0].tolist() == [4097] + [0] * (P - 1)


def test_a_batch_past_one_chunk_of_tiles(hooks):
    import sherman_amd as shm
    t = shm.Tree(arena_bytes=16 << 20, max_batch=1 << 14)
    for P, kind in ((8, "equal3"), (64, "narrow")):
        sp = splitters_for(P, kind)
        keys = keys_for(BIG, sp, P)
        for mode in (1, 2):
            check_bucket(run_bucket(t, hooks, keys, P, sp, mode), keys, P, sp)
    t.close()


@pytest.mark.parametrize("P", [1, 2, 3, 8, 64])
def test_no_splitters_is_route_bucket_bit_for_bit(tree, hooks, P):
    import sherman_amd as shm
    L = shm.lib()
    for n in (1, 1025, 8191):
        keys = keys_for(n, equal_splitters(P), n + P)
        kd = dev64(keys)
        outs = []
        for fn in ("plain", "null", "equal"):
            ko = torch.zeros(n, dtype=torch.int64, device="cuda")
            perm = torch.zeros(n, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(P, dtype=torch.int64, device="cuda")
            if fn == "plain":
                tree.route_bucket(kd, P, ko, perm, cnt)
            elif fn == "null":
                assert L.shm_route_bucket_bounds(tree.h, kd.data_ptr(), n, P, None, cnt.data_ptr(),
                                                 ko.data_ptr(), perm.data_ptr(), None) == 0
            else:  # the equal slices' own boundaries as splitters: the same owners
                tree.route_bucket(kd, P, ko, perm, cnt, splitters=equal_splitters(P))
            torch.cuda.synchronize()
            outs.append((cnt.cpu(), ko.cpu(), perm.cpu()))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], o))


@pytest.mark.parametrize("P,kind", [(2, "narrow"), (3, "wide"), (8, "equal3"), (8, "zero"),
                                    (16, "narrow"), (64, "equal3")])
def test_slot_placement_with_bounds(tree, hooks, P, kind):
    """Every key's spos lies in its owner's run and holds the key; the
    cursors are the owners' counts; nothing overflows at a capacity of n."""
    sp = splitters_for(P, kind)
    arr = (ctypes.c_uint64 * max(len(sp), 1))(*sp)
    for n in (1, 4095, 4097, 8191):
        keys = keys_for(n, sp, 13 * n + P)
        cap = n
        for mode in ((1, 2) if P <= 16 else (2,)):
            kd = dev64(keys)
            cursor = torch.zeros(P + 1, dtype=torch.int32, device="cuda")
            slots = torch.empty(P * cap, dtype=torch.int64, device="cuda")
            spos = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            assert hooks.shm__route_slots_bounds(tree.h, kd.data_ptr(), n, P, cap,
                                                 cursor.data_ptr(), slots.data_ptr(),
                                                 spos.data_ptr(), None, None, 1, arr, mode,
                                                 None) == 0
            torch.cuda.synchronize()
            own = owner(keys, sp)
            s = spos.cpu().numpy().view(np.uint32).astype(np.int64)
            sl = slots.cpu().numpy().view(U64)
            assert np.array_equal(s // cap, own), (n, mode)
            assert np.array_equal(sl[s], keys)
            assert np.unique(s).size == n
            cur = cursor.cpu().numpy()
            assert np.array_equal(cur[:P], np.bincount(own, minlength=P)) and cur[P] == 0
            for p in range(P):
                assert np.all(sl[p * cap + int(cur[p]):(p + 1) * cap] == U64(KEY_MAX))
    tree.synchronize()


def test_a_keymax_key_is_still_rejected_whole(tree, hooks):
    """The routed insert's bucketing with splitters: a batch holding kKeyMax
    routes nothing (every count 0) and the next synchronising call reports
    SHM_EINVAL, as with equal slices."""
    import sherman_amd as shm
    P, sp = 8, splitters_for(8, "narrow")
    arr = (ctypes.c_uint64 * 7)(*sp)
    keys = keys_for(3000, sp, 5)
    keys[1234] = U64(KEY_MAX)
    kd = dev64(keys)
    ko = torch.zeros(3000, dtype=torch.int64, device="cuda")
    perm = torch.zeros(3000, dtype=torch.int32, device="cuda")
    cnt = torch.full((P,), -1, dtype=torch.int64, device="cuda")
    assert hooks.shm__route_bucket_insert(tree.h, kd.data_ptr(), 3000, P, arr, cnt.data_ptr(),
                                          ko.data_ptr(), perm.data_ptr(), None) == 0
    with pytest.raises(shm.ShermanError) as e:
        tree.synchronize()
    assert e.value.rc == shm.SHM_EINVAL
    assert cnt.cpu().tolist() == [0] * P
    tree.last_error(reset=True)
    # the plain bucketing still groups it (by the owner rule: the last shard)
    got = run_bucket(tree, hooks, keys, P, sp, None)
    check_bucket(got, keys, P, sp)
    tree.synchronize()
