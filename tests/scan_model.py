"""Host model of the ordered scans (shm_scan_batch), in numpy, sharing no
code with the library: over a tree's contents sorted by key, scan (lo, hi,
limit) is the slice searchsorted(lo, 'left') : searchsorted(hi, 'right') cut
to `limit`.  Keys compare as unsigned 64-bit words."""
import numpy as np

U64 = np.uint64
KEY_MAX = (1 << 64) - 1


class ScanModel:
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

    def bounds(self, lo, hi=None):
        """(first, end) positions of every scan's matches."""
        lo = np.ascontiguousarray(lo, dtype=U64)
        a = np.searchsorted(self.keys, lo, side="left")
        if hi is None:
            b = np.full(lo.size, self.keys.size, dtype=a.dtype)
        else:
            hi = np.ascontiguousarray(hi, dtype=U64)
            b = np.searchsorted(self.keys, hi, side="right")
        # no stored key equals KEY_MAX: a scan from it is empty by definition
        b = np.where(lo == U64(KEY_MAX), a, b)
        return a, np.maximum(a, b)

    def scan(self, lo, limit, hi=None):
        """(counts[n], keys[n, limit], vals[n, limit], written[n, limit]):
        the pairs each scan returns and which words of its row it writes."""
        a, b = self.bounds(lo, hi)
        counts = np.minimum(b - a, limit).astype(np.int64)
        col = np.arange(limit, dtype=np.int64)[None, :]
        written = col < counts[:, None]
        idx = np.where(written, a[:, None] + col, 0)
        if self.keys.size == 0:
            z = np.zeros((a.size, limit), dtype=U64)
            return counts, z, z.copy(), written
        keys = np.where(written, self.keys[idx], U64(0))
        vals = np.where(written, self.vals[idx], U64(0))
        return counts, keys, vals, written
