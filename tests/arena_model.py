"""Host-side judge of what an insert chunk left behind when the page arena ran
out (SHM_ENOMEM), in numpy, sharing no code with the library; and the chunk
the tall-tree and arena tests apply (hot_chunk).

shm_insert_batch promises that only the splits that did not fit are left
unapplied.  A leaf's ops are applied together or not at all, so after a
failed chunk every key is in one of two states: the one it had before the
chunk or the one the whole chunk would have given it.  classify_outcome holds
a tree's contents to exactly that, and to the ops that must not be missing.
"""
import numpy as np

import image_builder as ib

U64 = np.uint64


class OutcomeError(AssertionError):
    """classify_outcome's verdict; kind is "extra", "untouched", "third_value"
    or "must_apply", keys the offending keys"""

    def __init__(self, kind, keys, text):
        self.kind = kind
        self.keys = keys
        super().__init__(f"{kind}: {text}")


def _pairs(kv, what):
    k = np.asarray(kv[0], dtype=U64).reshape(-1)
    v = np.asarray(kv[1], dtype=U64).reshape(-1)
    assert k.size == v.size, what
    o = np.argsort(k, kind="stable")
    k, v = k[o], v[o]
    assert k.size < 2 or (k[1:] != k[:-1]).all(), f"{what}: a key twice"
    assert (v != U64(0)).all(), f"{what}: a stored key without a value"
    return k, v


def _state(universe, kv):
    """the value of each key of the universe, 0 where it is not stored"""
    k, v = kv
    if k.size == 0:
        return np.zeros(universe.size, dtype=U64)
    at = np.minimum(np.searchsorted(k, universe), k.size - 1)
    return np.where(k[at] == universe, v[at], U64(0))


def classify_outcome(before, after, T, must_apply):
    """before, after, T: (keys, values) of the contents without the chunk,
    with all of it (from a tree with room), and as found.  must_apply: keys of
    the ops that have to be in their `after` state.

    Raises OutcomeError when
      a key of T is stored neither before nor after ("extra"),
      a key the chunk leaves as it was (same state before and after) is in
        another state ("untouched": lost, changed or resurrected),
      a key is in a state that is neither its before nor its after one
        ("third_value"),
      a key of must_apply is not in its after state ("must_apply").
    Returns the counts of the keys the chunk changes: {"applied",
    "unapplied", "new_stored", "new_not_stored"} (new: absent before, stored
    after)."""
    before, after, T = _pairs(before, "before"), _pairs(after, "after"), _pairs(T, "T")
    must = np.unique(np.asarray(must_apply, dtype=U64).reshape(-1))
    uni = np.unique(np.concatenate([before[0], after[0], T[0], must]))
    sb, sa, st = _state(uni, before), _state(uni, after), _state(uni, T)

    def fail(kind, mask, text):
        bad = uni[mask]
        lines = [f"key={int(k):#x} before={int(b):#x} after={int(a):#x} found={int(t):#x}"
                 for k, b, a, t in zip(bad[:8], sb[mask][:8], sa[mask][:8], st[mask][:8])]
        raise OutcomeError(kind, bad, f"{bad.size} keys {text}:\n" + "\n".join(lines))

    extra = (st != 0) & (sb == 0) & (sa == 0)
    if extra.any():
        fail("extra", extra, "stored that neither state holds")
    untouched = (sb == sa) & (st != sb)
    if untouched.any():
        fail("untouched", untouched, "the chunk does not change differ from before")
    third = (st != sb) & (st != sa)
    if third.any():
        fail("third_value", third, "in a state that is neither before nor after")
    m = np.isin(uni, must) & (st != sa)
    if m.any():
        fail("must_apply", m, "of ops that must be applied are not in their after state")
    changed = sb != sa
    new = changed & (sb == 0)
    return {"applied": int((changed & (st == sa)).sum()),
            "unapplied": int((changed & (st == sb)).sum()),
            "new_stored": int((new & (st == sa)).sum()),
            "new_not_stored": int((new & (st == sb)).sum())}


def hot_chunk(info):
    """40 absent keys inside the hot leaf's fences, 10 deletes and 10
    overwrites of keys in thin leaves elsewhere, and two in-chunk duplicates
    (a new key written twice, an overwritten key written again): keys,
    values (0 deletes; the last writer of a key wins)."""
    k = info["keys"]
    inside = (k >= U64(info["hot_lo"])) & (k < U64(info["hot_hi"]))
    hot, thin = k[inside], k[~inside]
    assert hot.size == ib.FULL_KEYS
    new = hot[:40] + U64(7)
    far = thin[np.linspace(0, thin.size - 1, 20).astype(np.int64)]
    dele, over = far[::2], far[1::2]
    keys = np.concatenate([new[:20], dele, over, new[20:], new[3:4], over[5:6]])
    vals = np.concatenate([new[:20] ^ U64(0x2222), np.zeros(10, dtype=U64), over ^ U64(0x3333),
                           new[20:] ^ U64(0x2222), new[3:4] ^ U64(0x4444), over[5:6] ^ U64(0x5555)])
    assert keys.size == 62 and np.unique(keys).size == 60
    return keys, vals
