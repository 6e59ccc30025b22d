"""shm_tree_set_key_range on a live tree of narrow keys.

One tree of 20,000 keys to_key(i) % 2^26 created with key_bits = 64: every
key shares directory entry 0, so every get starts at the root.  After
set_key_range(min, ceil(log2(span))) the same gets, misses, scans and
descending scans still match the oracle, keys outside the hint are still
stored and found, the rebuilt directory verifies (on the device and against
tests/dir_model.py), its entry count reflects the new range, and at most 5 %
of the gets start without a leaf summary -- a bound the model directory over
these keys meets as well (checked here before the device's figure)."""
import numpy as np
import pytest
import torch

from dir_model import Directory, Image, check_tree, fresh_usable

pytestmark = pytest.mark.gpu

U64 = np.uint64
SPACE = 1 << 26
N = 20000


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def gets(t, q):
    qd = dev64(q)
    v = torch.empty_like(qd)
    f = torch.empty(q.size, dtype=torch.uint8, device="cuda")
    t.search_batch(qd, v, f)
    t.synchronize()
    return v.cpu().numpy().view(U64), f.cpu().numpy()


def scans_match(t, ref, lo, hi, limit=64):
    c, k, v = t.scan_batch(dev64(lo), limit, hi=dev64(hi)).result()
    rc, rk, rv = t.rscan_batch(dev64(hi), limit, lo=dev64(lo)).result()
    c, k, v = c.cpu().numpy(), k.cpu().numpy().view(U64), v.cpu().numpy().view(U64)
    rc, rk, rv = rc.cpu().numpy(), rk.cpu().numpy().view(U64), rv.cpu().numpy().view(U64)
    keys, vals = ref
    for i in range(lo.size):
        a = np.searchsorted(keys, lo[i], side="left")
        b = np.searchsorted(keys, hi[i], side="right")
        m = min(limit, max(b - a, 0))
        assert c[i] == m and rc[i] == m, (i, c[i], rc[i], m)
        assert np.array_equal(k[i, :m], keys[a:a + m]) and np.array_equal(v[i, :m], vals[a:a + m])
        assert np.array_equal(rk[i, :m], keys[a:b][::-1][:m])
        assert np.array_equal(rv[i, :m], vals[a:b][::-1][:m])


def test_set_key_range_on_a_tree_of_narrow_keys():
    import sherman_amd as shm
    from oracle.pyoracle import OracleTree, to_key

    assert torch.cuda.is_available(), "GPU test without a GPU"
    torch.cuda.set_device(0)
    keys = np.unique(np.array([to_key(i) % SPACE for i in range(1, N + 1)], dtype=U64))
    vals = keys * U64(3) + U64(1)
    rng = np.random.default_rng(11)
    t = shm.Tree(arena_bytes=64 << 20, max_batch=1 << 15, key_bits=64)
    perm = rng.permutation(keys.size)
    t.insert_batch(dev64(keys[perm]), dev64(vals[perm]))
    orc = OracleTree(64 << 20)
    orc.apply_batch(keys, vals)
    # hits and a third misses; 1,000 of the misses lie outside [0, 2^26): no
    # hint over the stored keys covers those, so they always start at the root
    # (3.3 % of the batch, inside the 5 % the directory is held to below)
    q = np.concatenate([keys[rng.integers(0, keys.size, 20000)],
                        rng.integers(0, SPACE, 9000, dtype=np.uint64),
                        rng.integers(SPACE, (1 << 64) - 2, 1000, dtype=np.uint64)])
    rng.shuffle(q)
    ov, of = orc.search_batch(q)
    slo = np.concatenate([rng.integers(0, SPACE, 60, dtype=np.uint64), np.array([0, 0], dtype=U64)])
    shi = np.concatenate([slo[:60] + rng.integers(0, SPACE // 64, 60, dtype=np.uint64),
                          np.array([(1 << 64) - 2, 5], dtype=U64)])

    t.profile(on=True, index_stats=True)
    for _ in range(8):  # into the read phase: the directory form the gets settle on
        gv, gf = gets(t, q)
    assert np.array_equal(gv, ov) and np.array_equal(gf, of)
    t.index_stats(reset=True)
    gets(t, q)
    before = t.index_stats(reset=True)
    bits_before = t.dir_stats()["bits"]
    print("before:", before, "dir bits", bits_before)
    # every key below 2^26 shares directory entry 0, which no leaf list can
    # cover: every get of such a key starts at the root (the 1,000 gets drawn
    # from the whole key space fall into other entries)
    narrow = int((q < U64(SPACE)).sum())
    assert narrow == 29000
    assert before["gets"] == q.size and before["start_internal"] == narrow
    scans_match(t, (keys, vals), slo, shi)

    span = int(keys[-1] - keys[0]) + 1
    bits = max(1, (span - 1).bit_length())
    t.set_key_range(int(keys[0]), bits)
    assert t.dir_stats()["form"] == "none"  # dropped: the next reader rebuilds it
    for _ in range(8):
        gv, gf = gets(t, q)
        assert np.array_equal(gv, ov) and np.array_equal(gf, of)
    scans_match(t, (keys, vals), slo, shi)
    ds = t.dir_stats()
    assert ds["form"] != "none" and ds["bits"] <= bits
    ent, info = t.dir_dump()
    assert info["lo"] == int(keys[0]) and info["shift"] == bits - ds["bits"]
    assert ent.shape[0] == 1 << ds["bits"]
    # the model first: a fresh directory of this shape over these pages sends
    # at most 5 % of the gets to a start without a leaf summary
    im = Image(*t.dump_image())
    d = Directory(ent, info["lo"], info["shift"])
    p, cov = d.prefix_of(q)
    model_bad = int((~cov).sum() + (~fresh_usable(im, d, p[cov])).sum())
    print("model: gets without a usable entry", model_bad, "of", q.size)
    assert model_bad <= 0.05 * q.size
    bad, checked = check_tree(t, keys, vals)
    assert not bad, bad[:4]
    assert sum(checked.values()) > 0
    v = t.dir_verify()
    assert v["checked"] > 0 and v["bad_lists"] == v["bad_pairs"] == v["bad_fps"] == v["bad_vals"] == 0
    t.index_stats(reset=True)
    gets(t, q)
    after = t.index_stats(reset=True)
    print("after:", after, "dir bits", ds["bits"])
    assert after["start_internal"] <= 0.05 * q.size

    # keys outside the hint (below key_lo is impossible here: above it) are
    # still stored and found, beside new keys inside it
    extra = np.unique(np.concatenate([rng.integers(SPACE, (1 << 64) - 2, 3000, dtype=np.uint64),
                                      rng.integers(0, SPACE, 3000, dtype=np.uint64)]))
    extra = np.setdiff1d(extra, keys)
    ev = extra ^ U64(0xABCDEF)
    t.insert_batch(dev64(extra), dev64(ev))
    orc.apply_batch(extra, ev)
    q2 = np.concatenate([extra, q])
    ov2, of2 = orc.search_batch(q2)
    for _ in range(3):
        gv, gf = gets(t, q2)
        assert np.array_equal(gv, ov2) and np.array_equal(gf, of2)
    allk = np.concatenate([keys, extra])
    allv = np.concatenate([vals, ev])
    o = np.argsort(allk)
    scans_match(t, (allk[o], allv[o]), slo, shi)
    v = t.dir_verify()
    assert v["bad_lists"] == v["bad_pairs"] == v["bad_fps"] == v["bad_vals"] == 0
    assert t.check()["keys"] == allk.size

    # normalisation as at create, and the errors
    t.set_key_range(12345, 0)  # 0 is read as 64, and 64 forces key_lo = 0
    gets(t, q2[:100])
    _, info = t.dir_dump()
    assert info["lo"] == 0 and info["shift"] == 64 - t.dir_stats()["bits"]
    with pytest.raises(shm.ShermanError) as e:
        t.set_key_range(0, 65)
    assert e.value.rc == shm.SHM_EINVAL
    tk = t.insert_order(dev64(extra[:10]), dev64(ev[:10]))
    with pytest.raises(shm.ShermanError) as e:
        t.set_key_range(0, 26)  # an ordered chunk waits for its apply
    assert e.value.rc == shm.SHM_EINVAL
    t.insert_apply(tk)
    t.set_key_range(int(keys[0]), bits)
    gv, gf = gets(t, q2)
    assert np.array_equal(gv, ov2) and np.array_equal(gf, of2)
    orc.close()
    t.close()
