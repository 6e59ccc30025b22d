"""Tree: one shard's B+tree behind the C-ABI, and the host-only planners."""
import ctypes

from ._abi import (DIR_FORMS, KEY_MAX, SHM_ENOSPC, SHM_FLAG_AUTO_SORT_GETS, SHM_FLAG_LEAF_DIR,
                   SHM_FLAG_PAGE_CHECK, SHM_FLAG_SORT_GETS, SHM_FLAG_TOP_LDS, ShmBulkPlan,
                   ShmConfig, ShmDirStats, ShmError, ShmIndexStats, ShmOrderStats, ShmProfile,
                   ShmStats, _as_dict, _check, _host_u64, _ptr, _range_bufs, _stream_ptr,
                   from_i64, lib, to_i64, u32, u64, vp)
from ._pending import PendingRange, PendingScan, PendingSlots, _StreamDone
from ._tree_hooks import _TreeHooks


def bulk_plan(n, leaf_fill=0, internal_fill=0):
    """The shape Tree.bulk_load gives n pairs (shm_bulk_plan; host arithmetic,
    no GPU): {"pages", "root_level", "level_pages": pages of level 0 ..
    root_level}.  Fills out of range or a tree taller than level 7 raise
    ShermanError(SHM_EINVAL)."""
    p = ShmBulkPlan()
    _check(lib().shm_bulk_plan(n, leaf_fill, internal_fill, ctypes.byref(p)), "bulk_plan")
    return {"pages": int(p.pages), "root_level": int(p.root_level),
            "level_pages": [int(x) for x in p.level_pages[:p.root_level + 1]]}


def rebalance_plan(counts, rank):
    """The even re-cut of len(counts) shards holding counts[p] pairs
    (shm_rebalance_plan; host arithmetic, no GPU): {"cut": P + 1 global
    positions, "send": pairs `rank` sends to each shard, "recv": pairs it
    receives from each}.  P = 0, P > 16 or rank >= P raise
    ShermanError(SHM_EINVAL)."""
    P = len(counts)
    c = _host_u64(counts)
    cut, send, recv = (u64 * (P + 1))(), (u64 * max(P, 1))(), (u64 * max(P, 1))()
    _check(lib().shm_rebalance_plan(c, P, rank, cut, send, recv), "rebalance_plan")
    return {"cut": [int(x) for x in cut], "send": [int(x) for x in send[:P]],
            "recv": [int(x) for x in recv[:P]]}


class Tree(_TreeHooks):
    """One shard's B+tree in HBM (reference: class Tree, include/Tree.h:42)."""

    def __init__(self, arena_bytes=1 << 30, max_batch=1 << 20, device=0,
                 node_id=0, sort_gets="auto", num_locks=None, sort_bits=16,
                 key_lo=0, key_bits=64, leaf_dir=True, top_lds=False, page_check=False):
        L = lib()
        cfg = ShmConfig()
        _check(L.shm_config_init(ctypes.byref(cfg)), "config")
        cfg.device = device
        cfg.node_id = node_id
        cfg.arena_bytes = arena_bytes
        cfg.max_batch = max_batch
        if num_locks is not None:
            cfg.num_locks = num_locks
        cfg.sort_bits = sort_bits
        cfg.key_lo = key_lo
        cfg.key_bits = key_bits
        # sort_gets: True (always order get batches by key), False (never),
        # "auto" (order dense batches, SHM_FLAG_AUTO_SORT_GETS)
        cfg.flags = ((SHM_FLAG_SORT_GETS if sort_gets is True else 0) |
                     (SHM_FLAG_AUTO_SORT_GETS if sort_gets == "auto" else 0) |
                     (SHM_FLAG_LEAF_DIR if leaf_dir else 0) |
                     (SHM_FLAG_TOP_LDS if top_lds else 0) |
                     (SHM_FLAG_PAGE_CHECK if page_check else 0))
        h = vp()
        _check(L.shm_tree_create(ctypes.byref(cfg), ctypes.byref(h)), "shm_tree_create")
        self.h = h
        self.device = device
        self.node_id = node_id
        self.max_batch = max_batch
        self._scratch = {}

    # -- lifecycle ----------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            lib().shm_tree_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- batched hot path (device tensors) -----------------------------------
    def search_batch(self, keys, vals_out, found_out=None, stream=None):
        _check(lib().shm_search_batch(self.h, _ptr(keys), keys.numel(),
                                      _ptr(vals_out), _ptr(found_out),
                                      _stream_ptr(stream)), "search_batch")

    def insert_batch(self, keys, vals, stream=None):
        """Apply the batch and return its status (one host synchronisation)."""
        _check(lib().shm_insert_batch(self.h, _ptr(keys), _ptr(vals), keys.numel(),
                                      _stream_ptr(stream)), "insert_batch")

    def insert_batch_async(self, keys, vals, stream=None):
        """Queue the batch on the device without a host wait; its status is
        raised by the next synchronising call (synchronize, insert_batch)."""
        _check(lib().shm_insert_batch_async(self.h, _ptr(keys), _ptr(vals), keys.numel(),
                                            _stream_ptr(stream)), "insert_batch_async")

    def insert_order(self, keys, vals, stream=None):
        """shm_insert_order: queue one chunk's ordering (n <= max_batch) on
        `stream`; returns the ticket for insert_apply.  keys / vals must stay
        alive until the ordering has run."""
        t = u32(0)
        _check(lib().shm_insert_order(self.h, _ptr(keys), _ptr(vals), keys.numel(),
                                      _stream_ptr(stream), ctypes.byref(t)), "insert_order")
        return int(t.value)

    def insert_apply(self, ticket, stream=None):
        """shm_insert_apply: queue the tree changes of an ordered chunk."""
        _check(lib().shm_insert_apply(self.h, ticket, _stream_ptr(stream)), "insert_apply")

    def mixed_batch(self, get_keys, vals_out, found_out, ins_keys, ins_vals, stream=None):
        """One mixed batch (shm_mixed_batch): the gets see the tree before the
        batch's inserts; the inserts are queued as insert_batch_async."""
        _check(lib().shm_mixed_batch(self.h, _ptr(get_keys), get_keys.numel(), _ptr(vals_out),
                                     _ptr(found_out) if found_out is not None else None,
                                     _ptr(ins_keys), _ptr(ins_vals), ins_keys.numel(),
                                     _stream_ptr(stream)), "mixed_batch")

    def del_batch(self, keys, stream=None):
        _check(lib().shm_del_batch(self.h, _ptr(keys), keys.numel(),
                                   _stream_ptr(stream)), "del_batch")

    def bulk_load(self, keys, vals, leaf_fill=0, internal_fill=0, stream=None):
        """Replace the tree's contents with the pairs (keys[i], vals[i])
        (shm_bulk_load): int64 device tensors holding the u64 bits, keys
        strictly ascending as UNSIGNED numbers.  Sorting is the caller's: an
        int64 sort puts keys >= 2^63 first (to_i64 / from_i64 convert single
        values; sort the u64 view, e.g. in numpy, or flip the top bit around
        a torch sort).  leaf_fill entries per leaf (0: 36), internal_fill
        records per internal page (0: 40); the shape is bulk_plan()'s.  Waits
        for the tree; unsorted input, KEY_MAX or a zero value raise
        ShermanError(SHM_EINVAL) and leave the tree as it was."""
        assert keys.numel() == vals.numel()
        _check(lib().shm_bulk_load(self.h, _ptr(keys), _ptr(vals), keys.numel(), leaf_fill,
                                   internal_fill, _stream_ptr(stream)), "bulk_load")

    def count(self, lo=0, hi=None, stream=None):
        """The number of valid pairs with lo <= key <= hi (hi None: KEY_MAX):
        shm_export's count pass alone.  Waits for the result."""
        n = u64(0)
        _check(lib().shm_export(self.h, lo, KEY_MAX if hi is None else hi, None, None, 0,
                                ctypes.byref(n), _stream_ptr(stream)), "count")
        return int(n.value)

    def export(self, lo=0, hi=None, keys=None, vals=None, stream=None):
        """Every valid pair with lo <= key <= hi (hi None: KEY_MAX) in
        ascending unsigned key order (shm_export): (keys, vals), int64 device
        tensors of length n holding the u64 bits, what one scan_batch(lo, hi)
        with an unbounded limit would return.  keys / vals may be passed in
        (at least n long; the slices [:n] are returned, no word past them is
        written; with only one given, only that array is exported and the
        other result is None), else both are allocated from a count-only
        call.  A buffer that is too small raises ShermanError(SHM_ENOSPC) with nothing
        written.  Read-only; waits for the result."""
        import torch
        hi = KEY_MAX if hi is None else hi
        sp = _stream_ptr(stream)
        n = u64(0)
        if keys is None and vals is None:
            m = self.count(lo, hi, stream)
            keys = torch.empty(m, dtype=torch.int64, device=f"cuda:{self.device}")
            vals = torch.empty(m, dtype=torch.int64, device=f"cuda:{self.device}")
        cap = min(x.numel() for x in (keys, vals) if x is not None)
        _check(lib().shm_export(self.h, lo, hi, _ptr(keys), _ptr(vals), cap, ctypes.byref(n), sp),
               "export")
        return (None if keys is None else keys[:n.value],
                None if vals is None else vals[:n.value])

    def compact(self, leaf_fill=0, internal_fill=0, stream=None):
        """Rebuild the tree from its own valid pairs (shm_compact): export,
        then bulk_load(leaf_fill, internal_fill); the shape is
        bulk_plan(count(), leaf_fill, internal_fill).  A rejected call
        (fills, a plan too tall or too large for the arena) raises and leaves
        the tree as it was.  Waits for the tree."""
        _check(lib().shm_compact(self.h, leaf_fill, internal_fill, _stream_ptr(stream)),
               "compact")

    # -- scans -----------------------------------------------------------------
    def range_query_batch(self, lo, hi, stream=None):
        """Batched inclusive scans [lo_i, hi_i]: (counts, values concatenated
        in query order), both on the device; one host synchronisation (the
        total).  Results are stream-ordered on `stream`."""
        import torch
        n = lo.numel()
        dev = lo.device
        cap = getattr(self, "_rq_cap", 1 << 16)
        counts, offs, vals = _range_bufs(n, cap, dev)
        total = u64(0)
        rc = lib().shm_range_query_batch(self.h, _ptr(lo), _ptr(hi), n, _ptr(counts),
                                         _ptr(offs), _ptr(vals), cap, ctypes.byref(total),
                                         _stream_ptr(stream))
        total = int(total.value)
        if rc == SHM_ENOSPC:
            vals = torch.empty(total, dtype=torch.int64, device=dev)
            rc = lib().shm_range_query(self.h, _ptr(lo), _ptr(hi), n, _ptr(counts),
                                       _ptr(offs), _ptr(vals), _stream_ptr(stream))
        _check(rc, "range_query_batch")
        self._rq_cap = max(cap, total + total // 4)
        return counts, vals[:total]

    def range_query_batch_async(self, lo, hi, stream=None):
        """range_query_batch without the host synchronisation (n <= max_batch):
        the scans are queued on `stream` and the returned PendingRange gives
        (counts, values) on .result().  The value buffer is sized from earlier
        totals (the first call on a handle runs synchronously to learn one);
        .result() raises SHM_ENOSPC if this batch's total outgrew it, which
        cannot be redone after later mutating calls."""
        import torch
        cap = getattr(self, "_rq_cap", None)
        if cap is None:
            return PendingRange(None, *self.range_query_batch(lo, hi, stream))
        n = lo.numel()
        dev = lo.device
        # _range_bufs written out: this runs once a step in a timed loop
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        offs = torch.empty(n, dtype=torch.int64, device=dev)
        vals = torch.empty(cap, dtype=torch.int64, device=dev)
        tot = torch.empty(2, dtype=torch.int64, device=dev)
        sp = _stream_ptr(stream)
        _check(lib().shm_range_query_batch_async(self.h, _ptr(lo), _ptr(hi), n, _ptr(counts),
                                                 _ptr(offs), _ptr(vals), cap, _ptr(tot), sp),
               "range_query_batch_async")
        return PendingRange(self, counts, vals, tot, _StreamDone(sp, dev))

    def range_query_slots(self, lo, hi, slot_cap, stream=None, vals=None, counts=None,
                          status=None):
        """Batched scans with a buffer per scan (shm_range_query_slots, the
        reference's Tree::range_query(from, to, buffer) per scan): queued on
        `stream` without a host wait.  Returns PendingSlots: .result() gives
        (counts, vals[n, slot_cap]); scan i's first min(counts[i], slot_cap)
        values are vals[i, :counts[i]].  vals / counts may be passed in
        (reused buffers); status (2 device words, zeroed by the caller)
        accumulates {scans past slot_cap, error bits} over calls."""
        import torch
        n = lo.numel()
        dev = lo.device
        if counts is None:
            counts = torch.empty(n, dtype=torch.int64, device=dev)
        if vals is None:
            vals = torch.empty((n, slot_cap), dtype=torch.int64, device=dev)
        assert vals.numel() >= n * slot_cap and counts.numel() >= n
        sp = _stream_ptr(stream)
        _check(lib().shm_range_query_slots(self.h, _ptr(lo), _ptr(hi), n, slot_cap, _ptr(counts),
                                           _ptr(vals), _ptr(status), sp),
               "range_query_slots")
        return PendingSlots(self, counts[:n], vals, slot_cap, status, _StreamDone(sp, dev))

    def _scan(self, call, what, start, end, limit, stream, keys, vals, counts, status):
        """scan_batch / rscan_batch: `call` is the library's entry point,
        which takes the bound a scan starts at, then the one that ends it."""
        import torch
        n = start.numel()
        dev = start.device
        if end is not None:
            assert end.numel() == n
        if counts is None:
            counts = torch.empty(n, dtype=torch.int64, device=dev)
        if keys is None:
            keys = torch.empty((n, limit), dtype=torch.int64, device=dev)
        if vals is None:
            vals = torch.empty((n, limit), dtype=torch.int64, device=dev)
        assert keys.numel() >= n * limit and vals.numel() >= n * limit and counts.numel() >= n
        sp = _stream_ptr(stream)
        _check(call(self.h, _ptr(start), _ptr(end), n, limit, _ptr(keys), _ptr(vals),
                    _ptr(counts), _ptr(status), sp), what)
        return PendingScan(self, counts[:n], keys, vals, limit, status, _StreamDone(sp, dev))

    def scan_batch(self, lo, limit, hi=None, stream=None, keys=None, vals=None, counts=None,
                   status=None):
        """Ordered scans with a count limit (shm_scan_batch): scan i is the
        first `limit` valid entries with lo[i] <= key <= hi[i] (hi None: no
        upper bound) in ascending unsigned key order, queued on `stream`
        without a host wait.  Returns PendingScan: .result() gives (counts,
        keys[n, limit], vals[n, limit]).  keys / vals / counts may be passed
        in (reused buffers); status (2 device words, zeroed by the caller)
        gets the device error bits ORed into status[1]."""
        return self._scan(lib().shm_scan_batch, "scan_batch", lo, hi, limit, stream, keys, vals,
                          counts, status)

    def rscan_batch(self, hi, limit, lo=None, stream=None, keys=None, vals=None, counts=None,
                    status=None):
        """Descending scans with a count limit (shm_rscan_batch): scan i is
        the first `limit` valid entries with lo[i] <= key <= hi[i] (lo None:
        no lower bound) in descending unsigned key order; hi[i] == KEY_MAX
        starts at the largest stored key.  Queued on `stream` without a host
        wait.  Returns PendingScan; buffers and status as in scan_batch."""
        return self._scan(lib().shm_rscan_batch, "rscan_batch", hi, lo, limit, stream, keys, vals,
                          counts, status)

    def _nearest(self, scan, keys, stream):
        """lower_bound_batch / floor_batch: `scan` with limit 1 from keys[i]."""
        import torch
        n = keys.numel()
        k = torch.zeros(n, dtype=torch.int64, device=keys.device)
        v = torch.zeros(n, dtype=torch.int64, device=keys.device)
        c, k, v = scan(keys, 1, stream=stream, keys=k, vals=v).result()
        return c != 0, k.view(-1), v.view(-1)

    def lower_bound_batch(self, keys, stream=None):
        """The first stored key >= keys[i] (a scan with limit 1): (found,
        key, value) tensors of n; key and value are 0 where found is False
        (nothing at or after keys[i]).  Waits for the result."""
        return self._nearest(self.scan_batch, keys, stream)

    def floor_batch(self, keys, stream=None):
        """The largest stored key <= keys[i] (a descending scan with limit 1):
        (found, key, value) tensors of n; key and value are 0 where found is
        False (nothing at or below keys[i]).  Waits for the result."""
        return self._nearest(self.rscan_batch, keys, stream)

    # -- order statistics ------------------------------------------------------
    def rank_batch(self, keys, stream=None, out=None, status=None):
        """The number of valid pairs below each key (shm_rank_batch): an int64
        device tensor of n holding the u64 bits, what count(0, keys[i] - 1)
        returns; KEY_MAX gives the total.  Answered from the order index: the
        first call after a change of the tree rebuilds it and waits, later
        ones queue one kernel on `stream` without a host wait.  out may be
        passed in; status (2 device words, zeroed by the caller) gets the
        device error bits ORed into status[1]."""
        import torch
        n = keys.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=keys.device)
        assert out.numel() >= n
        _check(lib().shm_rank_batch(self.h, _ptr(keys), n, _ptr(out), _ptr(status),
                                    _stream_ptr(stream)), "rank_batch")
        return out[:n]

    def count_batch(self, lo, hi, stream=None, out=None, status=None):
        """The number of valid pairs with lo[i] <= key <= hi[i]
        (shm_count_batch): an int64 device tensor of n, range_query's counts
        at a cost that does not grow with the ranges; lo > hi gives 0.
        Queueing, out and status as in rank_batch."""
        import torch
        n = lo.numel()
        assert hi.numel() == n
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=lo.device)
        assert out.numel() >= n
        _check(lib().shm_count_batch(self.h, _ptr(lo), _ptr(hi), n, _ptr(out), _ptr(status),
                                     _stream_ptr(stream)), "count_batch")
        return out[:n]

    def select_batch(self, ranks, stream=None, keys=None, vals=None, found=None, status=None):
        """The pair at each position of the key order, from 0
        (shm_select_batch): (keys, vals, found), element ranks[i] of export();
        past the end found is 0, the key KEY_MAX and the value 0.  Queueing
        and status as in rank_batch; keys / vals (int64) and found (uint8)
        may be passed in."""
        import torch
        n = ranks.numel()
        dev = ranks.device
        if keys is None:
            keys = torch.empty(n, dtype=torch.int64, device=dev)
        if vals is None:
            vals = torch.empty(n, dtype=torch.int64, device=dev)
        if found is None:
            found = torch.empty(n, dtype=torch.uint8, device=dev)
        assert keys.numel() >= n and vals.numel() >= n and found.numel() >= n
        _check(lib().shm_select_batch(self.h, _ptr(ranks), n, _ptr(keys), _ptr(vals), _ptr(found),
                                      _ptr(status), _stream_ptr(stream)), "select_batch")
        return keys[:n], vals[:n], found[:n]

    def order_stats(self):
        """The order index as it stands (shm_order_stats; host only, builds
        nothing): units, pairs, bytes, builds, last_build_ms."""
        st = ShmOrderStats()
        _check(lib().shm_order_stats(self.h, ctypes.byref(st)), "order_stats")
        return _as_dict(st)

    def quantile_keys(self, parts, stream=None):
        """The keys at positions floor(p * N / parts) for p = 1 .. parts - 1
        of the N stored pairs, the cuts of shm_rebalance_plan, by one select
        batch: an int64 device tensor of parts - 1 keys, empty when
        N < parts.  Waits for the result."""
        import torch
        dev = f"cuda:{self.device}"
        rank = self.rank_batch(self._word(KEY_MAX), stream)
        self.synchronize()
        total = from_i64(int(rank.item()))
        if parts < 2 or total < parts:
            return torch.empty(0, dtype=torch.int64, device=dev)
        pos = torch.tensor([p * total // parts for p in range(1, parts)], dtype=torch.int64,
                           device=dev)
        keys, _, _ = self.select_batch(pos, stream)
        self.synchronize()
        return keys

    # -- reference single-op API (Tree.h:47-54) -------------------------------
    def _word(self, x):
        """The u64 x as a one-element int64 tensor on the tree's device."""
        import torch
        return torch.tensor([to_i64(x)], dtype=torch.int64, device=f"cuda:{self.device}")

    def _dev(self, name, n):
        import torch
        t = self._scratch.get(name)
        if t is None or t.numel() < n:
            t = torch.empty(max(n, 1), dtype=torch.int64, device=f"cuda:{self.device}")
            self._scratch[name] = t
        return t[:n]

    def insert(self, k, v):
        self.insert_batch(self._word(k), self._word(v))

    def search(self, k):
        import torch
        vs = self._dev("sv", 1)
        fs = torch.empty(1, dtype=torch.uint8, device=f"cuda:{self.device}")
        self.search_batch(self._word(k), vs, fs)
        self.synchronize()
        return bool(fs.item()), from_i64(vs.item())

    def del_(self, k):
        self.del_batch(self._word(k))

    # -- introspection ---------------------------------------------------------
    def synchronize(self):
        _check(lib().shm_synchronize(self.h), "synchronize")

    def last_error(self, reset=False):
        """shm_last_error: the device error block as the last synchronising
        call that found bits read it (bits, the chunk that first saw them, the
        status returned, resumed chunks so far)."""
        e = ShmError()
        _check(lib().shm_last_error(self.h, ctypes.byref(e), 1 if reset else 0), "last_error")
        return _as_dict(e)

    def last_chunk(self):
        """Id of the last insert chunk queued (shm_last_chunk)."""
        return int(lib().shm_last_chunk(self.h))

    def stats(self):
        s = ShmStats()
        _check(lib().shm_stats(self.h, ctypes.byref(s)), "stats")
        return _as_dict(s)

    def check(self):
        a, b, c = u64(), u64(), u64()
        _check(lib().shm_check(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
               "check")
        return dict(leaves=a.value, internal=b.value, keys=c.value)

    def dump_image(self):
        import numpy as np
        used, root = u64(), u64()
        _check(lib().shm_dump_image(self.h, None, 0, ctypes.byref(used), ctypes.byref(root)),
               "dump")
        buf = np.zeros(used.value, dtype=np.uint8)
        _check(lib().shm_dump_image(self.h, buf.ctypes.data_as(vp), used.value,
                                    ctypes.byref(used), ctypes.byref(root)), "dump")
        return buf, root.value

    def load_image(self, image, root_ptr):
        import numpy as np
        image = np.ascontiguousarray(image, dtype=np.uint8)
        _check(lib().shm_load_image(self.h, image.ctypes.data_as(vp), image.nbytes,
                                    root_ptr), "load_image")

    def profile(self, on=True, index_stats=False):
        _check(lib().shm_profile_enable(self.h, (1 if on else 0) | (2 if index_stats else 0)),
               "profile_enable")

    def profile_read(self, reset=True):
        p = ShmProfile()
        _check(lib().shm_profile_read(self.h, ctypes.byref(p), 1 if reset else 0),
               "profile_read")
        return _as_dict(p)

    def index_stats(self, reset=True):
        """The get walk's index statistics (shm_index_stats; collected while
        profile(index_stats=True))."""
        st = ShmIndexStats()
        _check(lib().shm_index_stats(self.h, ctypes.byref(st), 1 if reset else 0), "index_stats")
        return _as_dict(st)

    def dir_stats(self):
        """The leaf directory: form ("none" / "fingerprints" / "pairs"),
        entries, device bytes, builds and their device time (shm_dir_stats)."""
        st = ShmDirStats()
        _check(lib().shm_dir_stats(self.h, ctypes.byref(st)), "dir_stats")
        d = _as_dict(st)
        d["form"] = DIR_FORMS.get(d["form"], str(d["form"]))
        return d

    # -- routing / generators ---------------------------------------------------
    def read_i64(self, t, stream=None):
        """A small device int64 tensor (<= 32 words) as a list of ints, via
        the zero-copy read-back (shm_read_words); CPU tensors via tolist()."""
        if t.device.type != "cuda":
            return t.tolist()
        n = t.numel()
        buf = (ctypes.c_int64 * n)()
        _check(lib().shm_read_words(self.h, _ptr(t), 8 * n, buf, _stream_ptr(stream)),
               "read_words")
        return list(buf)

    def route_bucket(self, keys, num_shards, keys_out, perm_out, counts_out, stream=None,
                     splitters=None):
        """Stable bucketing by owner.  splitters: num_shards - 1 ascending u64
        boundaries (Python ints or numpy u64, host values; repeats make empty
        shards), None: equal slices of 2^64."""
        if splitters is None:
            _check(lib().shm_route_bucket(self.h, _ptr(keys), keys.numel(), num_shards,
                                          _ptr(counts_out), _ptr(keys_out), _ptr(perm_out),
                                          _stream_ptr(stream)), "route_bucket")
            return
        if len(splitters) != num_shards - 1:
            raise ValueError("route_bucket: num_shards - 1 splitters")
        _check(lib().shm_route_bucket_bounds(self.h, _ptr(keys), keys.numel(), num_shards,
                                             _host_u64(splitters), _ptr(counts_out),
                                             _ptr(keys_out), _ptr(perm_out),
                                             _stream_ptr(stream)), "route_bucket_bounds")

    def set_key_range(self, key_lo, key_bits):
        """Change the key range hint of the live tree (shm_tree_set_key_range):
        exclusive and synchronising; the directory and the bucket table are
        rebuilt over [key_lo, key_lo + 2^key_bits) by the next reader.  Keys
        outside the hint are still stored and found."""
        _check(lib().shm_tree_set_key_range(self.h, from_i64(int(key_lo)), key_bits),
               "set_key_range")

    def route_permute(self, vals_in, perm, out, stream=None):
        _check(lib().shm_route_permute(self.h, _ptr(vals_in), _ptr(perm), vals_in.numel(),
                                       _ptr(out), _stream_ptr(stream)), "permute")

    def route_unpermute(self, vals_in, perm, out, stream=None, found=None):
        if found is not None:  # found[perm[i]] = vals_in[i] != 0 in the same pass
            _check(lib().shm_route_unpermute_found(self.h, _ptr(vals_in), _ptr(perm),
                                                   vals_in.numel(), _ptr(out), _ptr(found),
                                                   _stream_ptr(stream)), "unpermute")
            return
        _check(lib().shm_route_unpermute(self.h, _ptr(vals_in), _ptr(perm), vals_in.numel(),
                                         _ptr(out), _stream_ptr(stream)), "unpermute")

    def lock_bench(self, keys, stream=None):
        """Tree::lock_bench for every key: its lock word taken and released."""
        _check(lib().shm_lock_bench(self.h, _ptr(keys), keys.numel(), _stream_ptr(stream)),
               "lock_bench")

    def hash_keys(self, ids, out, keyspace=0, stream=None):
        _check(lib().shm_hash_keys(self.h, _ptr(ids), ids.numel(), keyspace, _ptr(out),
                                   _stream_ptr(stream)), "hash_keys")

    def gen_keys(self, first, n, out, keyspace=0, stream=None):
        _check(lib().shm_gen_keys(self.h, first, n, keyspace, _ptr(out),
                                  _stream_ptr(stream)), "gen_keys")
