"""Host model of the descending scans (shm_rscan_batch), in numpy, sharing no
code with the library: over a tree's contents sorted by key, scan (start,
stop, limit) is the positions b - 1, b - 2, ... down to a, cut to `limit`,
with a = searchsorted(stop, 'left') (0 without a stop) and b =
searchsorted(start, 'right').  Keys compare as unsigned 64-bit words."""
import numpy as np

U64 = np.uint64
KEY_MAX = (1 << 64) - 1


class RScanModel:
    def __init__(self, keys, vals):
        """keys / vals: the tree's valid pairs in any order (an oracle's
        dump()); the keys are unique."""
        keys = np.ascontiguousarray(keys, dtype=U64)
        vals = np.ascontiguousarray(vals, dtype=U64)
        order = np.argsort(keys, kind="stable")
        self.keys, self.vals = keys[order], vals[order]
        assert self.keys.size < 2 or (self.keys[1:] > self.keys[:-1]).all(), "duplicate keys"

    @classmethod
    def of(cls, oracle_tree):
        return cls(*oracle_tree.dump())

    def bounds(self, start, stop=None):
        """(a, b): scan i's matches are positions a[i] .. b[i] - 1."""
        start = np.ascontiguousarray(start, dtype=U64)
        b = np.searchsorted(self.keys, start, side="right")
        if stop is None:
            a = np.zeros(start.size, dtype=b.dtype)
        else:
            stop = np.ascontiguousarray(stop, dtype=U64)
            a = np.searchsorted(self.keys, stop, side="left")
        return np.minimum(a, b), b

    def scan(self, start, limit, stop=None):
        """(counts[n], keys[n, limit], vals[n, limit], written[n, limit]):
        the pairs each scan returns, largest key first, and which words of
        its row it writes."""
        a, b = self.bounds(start, stop)
        counts = np.minimum(b - a, limit).astype(np.int64)
        col = np.arange(limit, dtype=np.int64)[None, :]
        written = col < counts[:, None]
        idx = np.where(written, b[:, None] - 1 - col, 0)
        if self.keys.size == 0:
            z = np.zeros((a.size, limit), dtype=U64)
            return counts, z, z.copy(), written
        keys = np.where(written, self.keys[idx], U64(0))
        vals = np.where(written, self.vals[idx], U64(0))
        return counts, keys, vals, written
