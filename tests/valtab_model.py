"""Host model of the key-value bucket table (csrc/valtab.h), in numpy, sharing
no code with the kernels.

A bucket is a row of 16 u64: (key, value) of slots 0..7.  Bucket b covers the
keys [lo + (b << shift), lo + ((b + 1) << shift)).  A slot is live when its
value is not 0 and free when key and value are both 0 (a delete clears
both, so a free slot never carries a real key); a bucket is dead when the key
of slot 0 is KEY_MAX.  A dead bucket says nothing (its gets take the directory
path); every other bucket must hold exactly the stored (key, value) pairs of
its key range, each once.  Key 0 is the free slots' key and never uses the
table: it belongs to no bucket.
"""
import numpy as np

U64 = np.uint64
KEY_MAX = U64(0xFFFFFFFFFFFFFFFF)
SLOTS = 8


def bucket_of(keys, lo, shift):
    """bucket index of each key (int64; keys below lo give -1)"""
    keys = np.asarray(keys, dtype=U64)
    b = ((keys - U64(lo)) >> U64(shift)).astype(np.int64)
    return np.where((keys >= U64(lo)) & (keys != U64(0)), b, -1)


def dead(buckets):
    return buckets[:, 0] == KEY_MAX


def counts(keys, lo, shift, n):
    """stored keys per bucket"""
    b = bucket_of(keys, lo, shift)
    return np.bincount(b[(b >= 0) & (b < n)], minlength=n)


def check(buckets, lo, shift, keys, values):
    """Every violation as a tuple, [] when the image agrees with the stored
    (keys, values):
      ("wrong", b)      a bucket without the marker whose live pairs are not
                        exactly the stored pairs of its range
      ("duplicate", b)  a bucket without the marker holding a live key twice
      ("misplaced", b)  ... holding a live key of another bucket's range
      ("unmarked", b)   a bucket of more than 8 stored keys without the marker
      ("stale", b)      ... holding a slot without a value whose key is not 0
    """
    buckets = np.asarray(buckets, dtype=U64)
    n = buckets.shape[0]
    keys = np.asarray(keys, dtype=U64)
    values = np.asarray(values, dtype=U64)
    bad = []
    is_dead = dead(buckets)
    cnt = counts(keys, lo, shift, n)
    for b in np.nonzero((cnt > SLOTS) & ~is_dead)[0]:
        bad.append(("unmarked", int(b)))
    # the live pairs of the buckets without the marker, as sorted (bucket, key, value)
    sk = buckets[:, 0::2]
    sv = buckets[:, 1::2]
    live = (sv != U64(0)) & ~is_dead[:, None]
    for b in np.unique(np.nonzero((sv == U64(0)) & (sk != U64(0)) & ~is_dead[:, None])[0]):
        bad.append(("stale", int(b)))
    rows = np.nonzero(live)[0]
    tk, tv = sk[live], sv[live]
    home = bucket_of(tk, lo, shift)
    for b in np.unique(rows[home != rows]):
        bad.append(("misplaced", int(b)))
    o = np.lexsort((tk, rows))
    rows, tk, tv = rows[o], tk[o], tv[o]
    dup = (rows[1:] == rows[:-1]) & (tk[1:] == tk[:-1])
    for b in np.unique(rows[1:][dup]):
        bad.append(("duplicate", int(b)))
    # the stored pairs of the same buckets
    kb = bucket_of(keys, lo, shift)
    ok = (kb >= 0) & (kb < n)
    ok[ok] &= ~is_dead[kb[ok]]
    ek, ev, eb = keys[ok], values[ok], kb[ok]
    o = np.lexsort((ek, eb))
    ek, ev, eb = ek[o], ev[o], eb[o]
    wrong = set()
    if rows.size != eb.size or not (np.array_equal(rows, eb) and np.array_equal(tk, ek)
                                    and np.array_equal(tv, ev)):
        # per bucket: compare the two sorted lists
        got = {}
        for r, k, v in zip(rows.tolist(), tk.tolist(), tv.tolist()):
            got.setdefault(r, []).append((k, v))
        want = {}
        for r, k, v in zip(eb.tolist(), ek.tolist(), ev.tolist()):
            want.setdefault(r, []).append((k, v))
        for b in set(got) | set(want):
            if got.get(b, []) != want.get(b, []):
                wrong.add(b)
    for b in sorted(wrong):
        bad.append(("wrong", int(b)))
    return bad


def check_tree(t, keys, values):
    """check() on a tree's dump (Tree.vt_dump); ([], info) when clean"""
    buckets, info = t.vt_dump()
    return check(buckets, info["lo"], info["shift"], keys, values), info
