"""The insert batches of tests/test_gpu_order.py, one builder per case, each
with the path it is meant to take written as assertions on order_model.plan.

tests/test_order_model.py runs the assertions on the CPU (a generator that
drifts off its path fails there first); tests/test_gpu_order.py runs them
again before it gives the batch to the GPU.

Every batch carries duplicates of a key within the batch (across 2048-op
tiles where it has more than one), and about a tenth of its values are 0
(deletes) unless the case is about the values.  Values are unique per op
(a per-case salt and the op's index), so a wrong writer shows.
"""
import zlib
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

U64 = np.uint64
KEY_MAX = (1 << 64) - 1
HINT_LO = 1 << 40


@dataclass
class Case:
    name: str
    tree: str                 # "small" (max_batch 2^14) | "big" (max_batch 2^22)
    keys: np.ndarray
    vals: np.ndarray
    expect: Callable          # asserts on the Plan
    hint: Optional[tuple] = None  # (key_lo, key_bits) set for the case, None: the whole key space
    counts: Optional[tuple] = None  # the ordering's counts where the case pins them


def splitmix(ids):
    """splitmix64 of the ids: spread 64-bit keys"""
    z = np.asarray(ids, dtype=U64) + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    z = z ^ (z >> U64(31))
    z[z == U64(KEY_MAX)] = U64(12345)
    return z


def values(name, rng, n, del_frac=0.1):
    salt = U64(zlib.crc32(name.encode()) & 0xFFFFF)
    v = (salt << U64(40)) | np.arange(1, n + 1, dtype=U64)
    if del_frac >= 1.0:
        v[:] = 0
    elif del_frac > 0:
        v[rng.random(n) < del_frac] = 0
    return v


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def spread(rng, n, universe):
    """n draws from the first `universe` hashed keys (shared by all cases, so
    later cases overwrite and delete what earlier ones stored)"""
    return splitmix(rng.integers(0, max(universe, 1), n))


def set_byte(k, d, b):
    sh = U64(8 * d)
    return (k & ~(U64(255) << sh)) | (np.asarray(b, dtype=U64) << sh)


def rand56(rng, n):
    return rng.integers(0, 1 << 56, n, dtype=np.uint64)


def top(b):
    return U64(b) << U64(56)


# ---- sizes in tile mode -------------------------------------------------------

def size_case(n):
    def build(lim):
        name = f"size_{n}"
        rng = rng_of(name)
        keys = spread(rng, n, n // 2)
        if n >= 2:
            keys[-1] = keys[0]  # the same key in the first and the last tile
        vals = values(name, rng, n)

        def expect(p):
            assert p.mode == "tile" and p.tiles == -(-n // lim["tile"])
            assert not p.bins("radix") and not p.bins("bitonic")
        return Case(name, "small", keys, vals, expect)
    return build


# ---- the switch from tile mode to the coarse pass -----------------------------

def switch_case(n, groups, ctiles, lastg):
    def build(lim):
        name = f"switch_{n}"
        rng = rng_of(name)
        keys = spread(rng, n, n // 2)
        vals = values(name, rng, n)

        def expect(p):
            if groups == 1:
                assert p.mode == "tile" and p.tiles == lim["max_tiles"]
            else:
                assert (p.mode, p.groups, p.coarse_tiles, p.last_groups) == \
                    ("coarse", groups, ctiles, lastg), (p.mode, p.groups, p.coarse_tiles,
                                                        p.last_groups)
            assert len(p.bins("empty")) == 0
            if n <= (1 << 20) + 4096:
                # every bin in LDS: the coarse pass hands them over through bins[]
                assert len(p.bins("rank")) == lim["coarse"], p.cnt.max()
            else:
                assert len(p.bins("radix")) == lim["coarse"], p.cnt.min()
        return Case(name, "big", keys, vals, expect)
    return build


def coarse_big_bin(lim):
    """half the ops clustered in one top byte (a radix bin of seven passes),
    the rest spread (LDS bins read through bins[]); clustered keys repeated
    across the two groups of coarse tile 0 and across coarse tiles"""
    name = "coarse_big_bin"
    n = (1 << 20) + 1
    T = lim["tile"]
    rng = rng_of(name)
    keys = spread(rng, n, n // 2)
    cl = rng.random(n) < 0.5
    uni = top(0xC3) | rand56(rng, n // 4)
    keys[cl] = uni[rng.integers(0, uni.size, int(cl.sum()))]
    keys[:300] = uni[:300]
    keys[T:T + 300] = uni[:300]            # group 1 of coarse tile 0
    keys[2 * T:2 * T + 300] = uni[:300]    # coarse tile 1
    keys[n - 1] = uni[0]                   # the last dedup tile's only op
    vals = values(name, rng, n)

    def expect(p):
        assert (p.mode, p.groups) == ("coarse", 2)
        assert p.bins("radix") == [0xC3] and p.radix_bytes[0xC3] == (0, 1, 2, 3, 4, 5, 6)
        assert len(p.bins("rank")) == lim["coarse"] - 1
    return Case(name, "big", keys, vals, expect)


# ---- heavy hitters -------------------------------------------------------------

def same_key_case(n, last_delete):
    def build(lim):
        name = f"same_key_{n}_{'del' if last_delete else 'put'}"
        rng = rng_of(name)
        keys = np.full(n, splitmix(np.array([77]))[0], dtype=U64)
        vals = values(name, rng, n)
        vals[-1] = 0 if last_delete else 0xABCDEF  # the last op wins
        tiles = -(-n // lim["tile"])

        def expect(p):
            assert p.mode == ("tile" if tiles <= lim["max_tiles"] else "coarse")
            b = int(keys[0] >> U64(56))
            assert p.cnt[b] == tiles and p.distinct[b] == 1 and p.path[b] == "rank"
            assert len(p.bins("empty")) == lim["coarse"] - 1
        return Case(name, "small" if n <= (1 << 14) else "big", keys, vals, expect,
                    counts=(0, 1) if last_delete else (1, 0))
    return build


def zipf_case(lim):
    name = "zipf_514_tiles"
    n = 513 * lim["tile"] + 100
    rng = rng_of(name)
    keys = splitmix(rng.zipf(1.2, n) % (1 << 19))
    vals = values(name, rng, n)

    def expect(p):
        assert p.mode == "coarse" and p.tiles == 514 and p.groups == 2
        assert p.cnt.sum() < n * 3 // 4  # the tiles' dedup shrinks the heavy hitters
    return Case(name, "big", keys, vals, expect)


def deletes_case(frac):
    def build(lim):
        name = "all_deletes" if frac >= 1.0 else "no_deletes"
        n = 5000
        rng = rng_of(name)
        keys = spread(rng, n, n // 2)
        vals = values(name, rng, n, del_frac=frac)

        def expect(p):
            assert p.mode == "tile" and p.tiles == 3
        return Case(name, "small", keys, vals, expect)
    return build


# ---- bin size at kUniqCap ------------------------------------------------------

def bin_cap_case(kind):
    def build(lim):
        name = f"bin_cap_{kind}"
        T, CAP = lim["tile"], lim["uniq_cap"]
        assert CAP % T == 0
        nt = CAP // T
        rng = rng_of(name)
        B = 0x3B
        uni = np.unique(top(B) | rand56(rng, CAP + 64))
        uni = uni[rng.permutation(uni.size)]
        if kind == "repeat":
            # the last tile repeats the first tile's keys: cnt == CAP, fewer survivors
            keys = np.concatenate([uni[:(nt - 1) * T], uni[:T][::-1]])
        else:
            keys = uni[:CAP].copy()
            # the same key in different tiles, each tile still T distinct keys
            keys[(nt - 1) * T:(nt - 1) * T + 100] = keys[:100]
        if kind == "over":
            keys = np.concatenate([keys, uni[CAP:CAP + 1]])  # one more survivor, in a new tile
        n = keys.size
        vals = values(name, rng, n)
        if kind != "repeat":
            vals[(nt - 1) * T:(nt - 1) * T + 50] = 0  # the later op is the delete

        def expect(p):
            assert p.mode == "tile" and p.tiles == nt + (kind == "over")
            assert p.cnt[B] == CAP + (kind == "over")
            assert p.distinct[B] == {"at": CAP - 100, "over": CAP - 99, "repeat": CAP - T}[kind]
            assert p.sub_max[B] <= lim["sub_cap"], p.sub_max[B]
            if kind == "over":
                assert p.path[B] == "radix" and p.passes(B) == 7
                assert p.radix_bytes[B] == (0, 1, 2, 3, 4, 5, 6)
            else:
                assert p.path[B] == "rank"
        return Case(name, "small", keys, vals, expect)
    return build


# ---- sub-bucket size at kSubRankCap --------------------------------------------

def sub_case(nsub):
    def build(lim):
        name = f"sub_{nsub}"
        SUB = lim["sub_cap"]
        rng = rng_of(name)
        B, F = 0x91, 0x44
        uni = np.unique(top(B) | (U64(F) << U64(48)) | rng.integers(0, 1 << 48, nsub + 8,
                                                                    dtype=np.uint64))[:nsub]
        assert uni.size == nsub
        extra = spread(rng, 2600, 1200)
        extra = extra[(extra >> U64(56)) != U64(B)]
        keys = np.concatenate([uni, uni[rng.integers(0, nsub, 3 * nsub)], extra])
        keys = keys[rng.permutation(keys.size)]
        vals = values(name, rng, keys.size)

        def expect(p):
            assert p.mode == "tile" and p.tiles == 2
            assert p.distinct[B] == nsub and p.sub_max[B] == nsub
            assert p.path[B] == ("rank" if nsub <= SUB else "bitonic")
            assert p.bins("bitonic") == ([] if nsub <= SUB else [B]) and not p.bins("radix")
        return Case(name, "small", keys, vals, expect)
    return build


def sub_full_bitonic(lim):
    """kUniqCap distinct keys in one sub-bucket: the bitonic network at its
    full width; the duplicates live in other bins, before and after them"""
    name = "sub_full_bitonic"
    CAP = lim["uniq_cap"]
    rng = rng_of(name)
    B, F = 0xA7, 0x02
    uni = np.unique(top(B) | (U64(F) << U64(48)) | rng.integers(0, 1 << 48, CAP + 64,
                                                                dtype=np.uint64))[:CAP]
    uni = uni[rng.permutation(CAP)]
    extra = spread(rng, 1000, 400)
    extra = extra[(extra >> U64(56)) != U64(B)]
    keys = np.concatenate([extra[:500], uni, extra[500:]])  # duplicates in tiles 0 and 3
    vals = values(name, rng, keys.size)

    def expect(p):
        assert p.mode == "tile"
        assert p.cnt[B] == CAP and p.distinct[B] == CAP and p.sub_max[B] == CAP
        assert p.path[B] == "bitonic" and p.bitonic_m[B] == 8192
    return Case(name, "small", keys, vals, expect)


# ---- radix passes ---------------------------------------------------------------

RADIX_BASE = 0x6D_5A_17_C3_2E_81_F4_09


def radix_case(S):
    """a bin over the cap whose keys differ on exactly the bytes S (byte 7:
    under a hint whose range the keys lie past, so they all clamp into bin
    255)"""
    S = tuple(sorted(S))

    def build(lim):
        name = "radix_" + "".join(map(str, S))
        T, CAP = lim["tile"], lim["uniq_cap"]
        rng = rng_of(name)
        hint = (1 << 41, 16) if 7 in S else None
        if len(S) == 1:
            d = S[0]
            vals_d = np.arange(1 if d == 7 else 0, 256, dtype=U64)
            uni = set_byte(np.full(vals_d.size, RADIX_BASE, dtype=U64), d, vals_d)
            n = (CAP // uni.size + 6) * T
        else:
            uni = np.full(6000, RADIX_BASE, dtype=U64)
            for d in S:
                uni = set_byte(uni, d, rng.integers(0, 256, uni.size))
            if 7 in S:
                uni = uni[(uni >> U64(56)) != U64(0)]  # past lo + 2^16
            uni = np.unique(uni)
            n = 5 * T
        keys = uni[rng.integers(0, uni.size, n)]
        vals = values(name, rng, n)
        b = 255 if 7 in S else RADIX_BASE >> 56

        def expect(p):
            assert p.mode == "tile"
            assert p.bins("radix") == [b] and len(p.bins("empty")) == lim["coarse"] - 1
            assert p.radix_bytes[b] == S, p.radix_bytes
        return Case(name, "small" if n <= (1 << 14) else "big", keys, vals, expect, hint=hint)
    return build


# ---- key-range hint --------------------------------------------------------------

def hint_keys(rng, n, bits, uni):
    """thirds: below key_lo (key 0 among them), inside the range, past it
    (2^64 - 2 among them); each third drawn from `uni` distinct keys"""
    lo = HINT_LO
    below = rng.integers(0, lo, uni, dtype=np.uint64)
    below[0] = 0
    below[1] = lo - 1
    inside = U64(lo) + rng.integers(0, 1 << bits, uni, dtype=np.uint64)
    inside[0] = lo
    inside[1] = lo + (1 << bits) - 1
    past = rng.integers(lo + (1 << bits), KEY_MAX, uni, dtype=np.uint64)
    past[0] = KEY_MAX - 1
    past[1] = lo + (1 << bits)
    m = n // 3
    keys = np.concatenate([below[rng.integers(0, uni, m)], inside[rng.integers(0, uni, m)],
                           past[rng.integers(0, uni, n - 2 * m - 6)],
                           below[:2], inside[:2], past[:2]])
    return keys[rng.permutation(n)]


def hint_case(bits, coarse_mode=False):
    def build(lim):
        name = f"hint_{bits}" + ("_coarse" if coarse_mode else "")
        rng = rng_of(name)
        n = (1 << 20) + 1 if coarse_mode else 6000
        keys = hint_keys(rng, n, bits, n // 6)
        vals = values(name, rng, n)

        def expect(p):
            assert p.mode == ("coarse" if coarse_mode else "tile")
            assert p.cnt[0] > n // 8 and p.cnt[255] > n // 8  # the clamped keys
            if bits == 1:
                assert p.cnt[128] > 0  # key_lo + 1, the range's upper half
            if coarse_mode:
                # even pass counts in coarse-pass mode: the keys past the range
                # differ on all eight bytes, those below (with the range's first
                # slice) on bytes 0..5
                assert p.path[0] == "radix" and p.radix_bytes[0] == (0, 1, 2, 3, 4, 5)
                assert p.path[255] == "radix" and p.passes(255) == 8
                assert len(p.bins("rank")) >= 200
        return Case(name, "big" if coarse_mode else "small", keys, vals, expect,
                    hint=(HINT_LO, bits))
    return build


def cluster_one_leaf(lim):
    """about 290 000 new keys inside one stored leaf's range, a tenth of them
    deleted in the same chunk: the leaf splits into more than 4096 leaves
    whatever their fill, and the chunk's deletes, which start from the
    directory entry of before the split, have that many leaves to their
    right.  Four radix passes in tile mode."""
    name = "cluster_one_leaf"
    n = 1 << 19
    rng = rng_of(name)
    base = (U64(0x77) << U64(56)) | (U64(0x123456) << U64(32))
    uni = base + rng.integers(0, 1 << 30, 400000, dtype=np.uint64)
    keys = uni[rng.integers(0, uni.size, n)]
    vals = values(name, rng, n)

    def expect(p):
        assert p.mode == "tile" and p.tiles == 256
        assert p.bins("radix") == [0x77] and p.radix_bytes[0x77] == (0, 1, 2, 3)
        assert p.distinct[0x77] > 54 * 4096 / 0.85  # leaves at any fill, after the deletes
    return Case(name, "big", keys, vals, expect)


BUILDERS = {}


def _add(b, name):
    BUILDERS[name] = b


for _n in (1, 2, 2047, 2048, 2049, 3 * 2048 + 1):
    _add(size_case(_n), f"size_{_n}")
_add(switch_case(1 << 20, 1, 0, 0), f"switch_{1 << 20}")
_add(switch_case((1 << 20) + 1, 2, 257, 1), f"switch_{(1 << 20) + 1}")
_add(switch_case((1 << 20) + 2048 + 5, 2, 257, 2), f"switch_{(1 << 20) + 2048 + 5}")
_add(switch_case(3 * (1 << 20) + 77, 4, 385, 1), f"switch_{3 * (1 << 20) + 77}")
_add(coarse_big_bin, "coarse_big_bin")
for _n in (5000, (1 << 20) + 1):
    _add(same_key_case(_n, False), f"same_key_{_n}_put")
    _add(same_key_case(_n, True), f"same_key_{_n}_del")
_add(zipf_case, "zipf_514_tiles")
_add(deletes_case(1.0), "all_deletes")
_add(deletes_case(0.0), "no_deletes")
for _k in ("at", "over", "repeat"):
    _add(bin_cap_case(_k), f"bin_cap_{_k}")
_add(sub_case(64), "sub_64")
_add(sub_case(65), "sub_65")
_add(sub_full_bitonic, "sub_full_bitonic")
for _S in ((0,), (0, 1, 2), (0, 3, 6), (1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5, 6), (2, 5),
           (0, 1, 2, 3, 4, 5, 6, 7), (7,)):
    _add(radix_case(_S), "radix_" + "".join(map(str, _S)))
for _b in (24, 40, 1):
    _add(hint_case(_b), f"hint_{_b}")
_add(hint_case(24, True), "hint_24_coarse")
_add(cluster_one_leaf, "cluster_one_leaf")
