"""CShard: the routed multi-GPU calls behind the C-ABI (shm_shard_*)."""
import ctypes

from ._abi import (SHM_ENOSPC, _check, _hooks, _host_u64, _ptr, _range_bufs, _stream_ptr, lib,
                   u32, u64, vp)


class CShard:
    """A range shard of a multi-GPU tree behind the C-ABI (shm_shard_*): the
    routed get / insert / range scan (slots, RCCL all-to-all, the overflow
    rounds, local batch, gather) runs in C++ over its own RCCL
    communicators.  All ranks construct it together (ncclCommInitRank); rank
    0's unique id travels over `dist`."""

    @classmethod
    def local(cls, tree, group, rank):
        """Rank `rank` of a LocalGroup (test hook; call from that rank's
        thread: creation is a collective)."""
        self = cls.__new__(cls)
        h = vp()
        _check(_hooks().shm__shard_create_local(tree.h, group.h, rank, ctypes.byref(h)),
               "shard_create_local")
        self.h, self.tree, self.world, self.rank = h, tree, group.world, rank
        return self

    def __init__(self, tree, world, rank, dist, group=None):
        import torch
        L = lib()
        idb = torch.zeros(128, dtype=torch.uint8)
        if rank == 0:
            _check(L.shm_nccl_unique_id(idb.data_ptr(), 128), "nccl_unique_id")
        backend = dist.get_backend(group)
        t = idb.to(f"cuda:{tree.device}") if backend == "nccl" else idb
        dist.broadcast(t, 0, group=group)
        idb = t.cpu()
        h = vp()
        _check(L.shm_shard_create(tree.h, idb.data_ptr(), 128, world, rank, ctypes.byref(h)),
               "shard_create")
        self.h, self.tree, self.world, self.rank = h, tree, world, rank

    def close(self):
        if getattr(self, "h", None):
            lib().shm_shard_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def force_route(self, on=True):
        """Test hook (shm__shard_force_route): every get and insert takes the
        routed path through the transport even at world 1 (RCCL sends each
        run to this rank itself)."""
        _check(_hooks().shm__shard_force_route(self.h, 1 if on else 0), "force_route")

    def search(self, keys, vals_out, found_out, stream=None):
        _check(lib().shm_shard_search(self.h, _ptr(keys), keys.numel(), _ptr(vals_out),
                                      _ptr(found_out), _stream_ptr(stream)), "shard_search")

    def search_begin(self, keys, stream=None):
        tk = u32()
        _check(lib().shm_shard_search_begin(self.h, _ptr(keys), keys.numel(),
                                            _stream_ptr(stream), ctypes.byref(tk)),
               "shard_search_begin")
        return tk.value

    def search_end(self, ticket, vals_out, found_out):
        _check(lib().shm_shard_search_end(self.h, ticket, _ptr(vals_out), _ptr(found_out)),
               "shard_search_end")

    def insert(self, keys, vals, stream=None):
        _check(lib().shm_shard_insert(self.h, _ptr(keys), _ptr(vals), keys.numel(),
                                      _stream_ptr(stream)), "shard_insert")

    def range_query(self, lo, hi, n_cap=None, stream=None):
        """Routed scans [lo_i, hi_i]: (counts, values in key order across
        shards).  n_cap: the same on every rank, >= lo.numel() (default: the
        tree's max_batch // P, so every rank may pass any n up to it)."""
        import torch
        n, dev = lo.numel(), lo.device
        if n_cap is None:
            n_cap = self.tree.max_batch // self.world
        cap = getattr(self, "_rq_cap", 1 << 16)
        counts, offs, vals = _range_bufs(n, cap, dev)
        total = u64(0)
        rc = lib().shm_shard_range_query(self.h, _ptr(lo), _ptr(hi), n, n_cap, _ptr(counts),
                                         _ptr(offs), _ptr(vals), cap, ctypes.byref(total),
                                         _stream_ptr(stream))
        total = int(total.value)
        self._rq_cap = max(cap, total + total // 4)
        if rc == SHM_ENOSPC:
            # the exchange completed: copy its values into a buffer that fits
            # (local, no second collective)
            vals = torch.empty(self._rq_cap, dtype=torch.int64, device=dev)
            rc = lib().shm_shard_range_values(self.h, _ptr(vals), self._rq_cap,
                                              _stream_ptr(stream))
        _check(rc, "shard_range_query")
        return counts, vals[:total]

    def range_query_async(self, lo, hi, vals_cap, peer_cap, n_cap=None, stream=None,
                          status=None):
        """range_query with no host synchronisation (shm_shard_range_query_async):
        the values travel in fixed runs of peer_cap per peer.  Returns
        (counts, offsets, vals[vals_cap], status): status[0] the total,
        status[1] flags (nonzero: incomplete, repeat with range_query before
        any tree change), all written on `stream`."""
        import torch
        n, dev = lo.numel(), lo.device
        if n_cap is None:
            n_cap = self.tree.max_batch // self.world
        counts, offs, vals = _range_bufs(n, max(vals_cap, 1), dev)
        if status is None:
            status = torch.zeros(2, dtype=torch.int64, device=dev)
        _check(lib().shm_shard_range_query_async(self.h, _ptr(lo), _ptr(hi), n, n_cap,
                                                 _ptr(counts), _ptr(offs), _ptr(vals), vals_cap,
                                                 peer_cap, _ptr(status), _stream_ptr(stream)),
               "shard_range_query_async")
        return counts, offs, vals, status

    def synchronize(self):
        _check(lib().shm_shard_synchronize(self.h), "shard_synchronize")

    def set_splitters(self, splitters):
        """The shards' boundaries b[1 .. P - 1] (shm_shard_set_splitters):
        world - 1 ascending u64 values, the same on every rank (checked);
        None: back to equal slices.  Moves no data."""
        if splitters is not None and len(splitters) != self.world - 1:
            raise ValueError("set_splitters: world - 1 splitters")
        _check(lib().shm_shard_set_splitters(self.h, _host_u64(splitters)), "shard_set_splitters")

    def splitters(self):
        """The current boundaries b[1 .. P - 1] as Python ints (the equal
        slices' when none are set)."""
        out = (u64 * max(self.world - 1, 1))()
        _check(lib().shm_shard_get_splitters(self.h, out), "shard_get_splitters")
        return [int(x) for x in out[:self.world - 1]]

    def rebalance(self, leaf_fill=0, internal_fill=0, stream=None):
        """Re-cut the stored pairs evenly over the shards and move them
        (shm_shard_rebalance; collective, exclusive, synchronising).  Returns
        this rank's new pair count."""
        n = u64(0)
        _check(lib().shm_shard_rebalance(self.h, leaf_fill, internal_fill, ctypes.byref(n),
                                         _stream_ptr(stream)), "shard_rebalance")
        return int(n.value)
