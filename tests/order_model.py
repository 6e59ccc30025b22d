"""Host model of the insert ordering (isort.hip, partition.hip's coarse pass).

order()  what the ordering must produce for a chunk: the last writer per key
         in batch order, upserts and deletes apart, both ascending.
plan()   which code the device takes for the chunk: tile mode or the coarse
         pass, and per coarse bin the LDS rank finish, the LDS bitonic finish
         or the radix sort through global scratch with its passes.
apply()  a sorted key / value image updated by an ordered chunk.

Numpy only; shares no code with the library.  The thresholds come from the
library (sherman_amd.order_limits()), so the model follows a retuned constant.
"""
from dataclasses import dataclass, field

import numpy as np

U64 = np.uint64
KEY_MAX = (1 << 64) - 1


def order(keys, vals):
    """(uk, uv, dk): for every distinct key its last op in batch order; a
    value of 0 is a delete.  uk / dk ascending as unsigned numbers."""
    keys = np.asarray(keys, dtype=U64)
    vals = np.asarray(vals, dtype=U64)
    assert keys.shape == vals.shape and keys.ndim == 1
    if keys.size == 0:
        e = np.zeros(0, dtype=U64)
        return e, e.copy(), e.copy()
    idx = np.argsort(keys, kind="stable")  # equal keys stay in batch order
    ks = keys[idx]
    last = np.ones(ks.size, dtype=bool)
    last[:-1] = ks[1:] != ks[:-1]
    k, v = ks[last], vals[idx][last]
    up = v != U64(0)
    return k[up], v[up], k[~up]


def apply(sk, sv, uk, uv, dk):
    """The sorted image (sk, sv) after the ordered chunk: upserts written,
    deletes gone."""
    keep = ~np.isin(sk, uk) & ~np.isin(sk, dk)
    k = np.concatenate([sk[keep], uk])
    v = np.concatenate([sv[keep], uv])
    o = np.argsort(k, kind="stable")
    return k[o], v[o]


def rel_key(keys, key_lo, key_bits):
    """device_common.h rel_key: a key's offset in [key_lo, key_lo + 2^key_bits)
    scaled to 64 bits; 0 below the range, 2^64 - 1 past it."""
    keys = np.asarray(keys, dtype=U64)
    if key_bits >= 64:
        return keys.copy()
    lo = U64(key_lo)
    d = keys - lo  # wraps below lo; those are replaced
    inside = (d >> U64(key_bits)) == U64(0)
    out = np.where(inside, d << U64(64 - key_bits), U64(KEY_MAX))
    return np.where(keys < lo, U64(0), out).astype(U64)


@dataclass
class Plan:
    n: int
    mode: str            # "tile" | "coarse"
    tiles: int           # dedup tiles of kIsortTile ops
    groups: int          # dedup tiles per coarse tile (1 in tile mode)
    coarse_tiles: int    # coarse tiles (0 in tile mode)
    last_groups: int     # dedup tiles in the last coarse tile
    cnt: np.ndarray      # per bin: sum over dedup tiles of the tile's distinct keys
    distinct: np.ndarray  # per bin: distinct keys of the chunk
    sub_max: np.ndarray  # per bin: the largest fine sub-bucket of distinct keys
    path: list           # per bin: "empty" | "rank" | "bitonic" | "radix"
    radix_bytes: dict = field(default_factory=dict)  # radix bin -> bytes its keys differ on
    bitonic_m: dict = field(default_factory=dict)    # bitonic bin -> width of the network

    def bins(self, path):
        return [b for b, p in enumerate(self.path) if p == path]

    def passes(self, b):
        return len(self.radix_bytes[b])


def plan(keys, key_lo, key_bits, limits, skip_pad=False):
    """The path the device takes for the chunk `keys` under the hint (key_lo,
    key_bits).  limits: sherman_amd.order_limits().  skip_pad: KEY_MAX keys
    are slot padding (no ops), as in a routed insert."""
    keys = np.asarray(keys, dtype=U64)
    T, MT, CAP, SUB = limits["tile"], limits["max_tiles"], limits["uniq_cap"], limits["sub_cap"]
    NC, NF = limits["coarse"], limits["fine"]
    assert NC == 256 and NF == 256, "the bins are the top two bytes of rel_key"
    if key_bits >= 64 or key_bits == 0:
        key_lo, key_bits = 0, 64
    n = keys.size
    tiles = (n + T - 1) // T
    if tiles <= MT:
        mode, groups, ctiles, lastg = "tile", 1, 0, 0
    else:
        mode = "coarse"
        groups = (tiles + MT - 1) // MT
        ctiles = (tiles + groups - 1) // groups
        lastg = tiles - (ctiles - 1) * groups
    tid = np.arange(n, dtype=np.int64) // T
    if skip_pad:
        real = keys != U64(KEY_MAX)
        keys, tid = keys[real], tid[real]
    # one survivor per (dedup tile, key)
    o = np.lexsort((keys, tid))
    tk, tt = keys[o], tid[o]
    first = np.ones(tk.size, dtype=bool)
    first[1:] = (tk[1:] != tk[:-1]) | (tt[1:] != tt[:-1])
    surv = tk[first]
    sbin = (rel_key(surv, key_lo, key_bits) >> U64(56)).astype(np.int64)
    cnt = np.bincount(sbin, minlength=NC)
    dk = np.unique(keys)
    drel = rel_key(dk, key_lo, key_bits)
    dbin = (drel >> U64(56)).astype(np.int64)
    distinct = np.bincount(dbin, minlength=NC)
    sub = np.bincount((drel >> U64(48)).astype(np.int64), minlength=NC * NF).reshape(NC, NF)
    sub_max = sub.max(axis=1)
    path, rbytes, bm = [], {}, {}
    for b in range(NC):
        if cnt[b] == 0:
            path.append("empty")
        elif cnt[b] > CAP:
            path.append("radix")
            kb = dk[dbin == b]  # the bin's cnt keys are these, some repeated
            rbytes[b] = tuple(d for d in range(8)
                              if np.unique((kb >> U64(8 * d)) & U64(255)).size > 1)
        elif sub_max[b] > SUB:
            path.append("bitonic")
            m = 2
            while m < distinct[b]:
                m <<= 1
            bm[b] = m
        else:
            path.append("rank")
    return Plan(n, mode, tiles, groups, ctiles, lastg, cnt, distinct, sub_max, path, rbytes, bm)
