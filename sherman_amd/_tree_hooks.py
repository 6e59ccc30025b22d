"""Test hooks and diagnostics (the shm__* calls of _abi._HOOKS): the Tree
methods tests and tools use to steer and inspect the library's internals, and
the module-level hooks.  None of them is API a caller may rely on."""
import ctypes

from ._abi import DIR_FORMS, _check, _hooks, _ptr, _stream_ptr, from_i64, u64, vp


class _TreeHooks:
    """The hooks of a Tree (mixed into it; they use its handle self.h)."""

    def dir_config(self, maint=None, mem_limit=0):
        """Test hook (shm__dir_config): directory upkeep by the chunks on /
        off (None: as is; "always": every chunk, also those with no search
        since the last one) and a byte cap on directory allocations."""
        m = -1 if maint is None else 2 if maint == "always" else int(bool(maint))
        _check(_hooks().shm__dir_config(self.h, m, mem_limit), "dir_config")

    def get_forms(self, coop=None, pack=None):
        """Test hook (shm__get_forms): the batched get's forms behind a
        bucket table for this tree's later launches, as SHM_GET_COOP and
        SHM_GET_PACK set them when the tree is created (None: as is)."""
        _check(_hooks().shm__get_forms(self.h, -1 if coop is None else int(bool(coop)),
                                       -1 if pack is None else int(bool(pack))), "get_forms")

    def seq_jump(self, which, value):
        """Test hook (shm__seq_jump): move the insert chunk counter ("chunk")
        or the scan counter ("scan") forward to `value`, as if that many
        chunks or scans without effect had run (tree.cpp lists every word it
        sets).  Waits for the tree; ShermanError(SHM_EINVAL) while ordered
        chunks are pending or when value is below the counter."""
        _check(_hooks().shm__seq_jump(self.h, {"chunk": 0, "scan": 1}[which], value), "seq_jump")

    def order_read(self, ticket, n):
        """Test hook (shm__order_read): the ordered chunk of an outstanding
        insert_order ticket of n ops, as insert_apply will read it: (uk, uv,
        dk, counts), numpy uint64 arrays (upsert keys ascending with their
        values, delete keys ascending) and counts = (upserts, deletes).  Waits
        for the ordering; the ticket stays outstanding.  Any other ticket
        raises ShermanError(SHM_EINVAL)."""
        import numpy as np
        uk, uv, dk = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
        c = (u64 * 2)()
        _check(_hooks().shm__order_read(self.h, ticket, uk.ctypes.data_as(vp),
                                        uv.ctypes.data_as(vp), dk.ctypes.data_as(vp), c),
               "order_read")
        nu, nd = int(c[0]), int(c[1])
        return uk[:nu], uv[:nu], dk[:nd], (nu, nd)

    def insert_batch_padded(self, keys, vals, stream=None):
        """Test hook (shm__insert_batch_padded): a routed insert's received
        slots queued as insert_batch_async of one chunk, KEY_MAX keys being
        slot padding that is skipped."""
        _check(_hooks().shm__insert_batch_padded(self.h, _ptr(keys), _ptr(vals), keys.numel(),
                                                 _stream_ptr(stream)), "insert_batch_padded")

    def dir_verify(self):
        """Diagnostics (shm__dir_verify): every directory entry the walks
        trust checked against the tree as it is now."""
        out = (u64 * 10)()
        _check(_hooks().shm__dir_verify(self.h, out), "dir_verify")
        return {"checked": out[0], "bad_lists": out[1], "bad_pairs": out[2], "bad_fps": out[3],
                "first_bad": [x - 1 for x in out[4:8] if x],
                "vals_checked": out[8], "bad_vals": out[9]}

    def dir_dump(self):
        """Test hook (shm__dir_dump): the raw directory as an (n, 16) uint32
        array (one 64 B entry per row; n == 0 while no directory is valid)
        and {"lo", "shift", "form"}: entry p covers the keys
        [lo + (p << shift), lo + ((p + 1) << shift))."""
        import numpy as np
        info = (u64 * 4)()
        _check(_hooks().shm__dir_dump(self.h, None, 0, info), "dir_dump")
        ent = np.zeros((int(info[0]), 16), dtype=np.uint32)
        if info[0]:
            _check(_hooks().shm__dir_dump(self.h, ent.ctypes.data_as(vp), info[0], info),
                   "dir_dump")
            assert info[0] == ent.shape[0]
        return ent, {"lo": int(info[1]), "shift": int(info[2]),
                     "form": DIR_FORMS.get(int(info[3]) if info[0] else 0, str(info[3]))}

    def side_dump(self, pages=None):
        """Test hook (shm__side_dump): the side state of the first `pages`
        arena pages (None: the pages in use): the leaf summary lines as a
        (pages, 64) uint8 array, the occupancy bounds as a (pages,) uint8
        array, and {"next_page", "cap_pages"}.  pages may reach past
        next_page, up to the arena's pages."""
        import numpy as np
        info = (u64 * 2)()
        _check(_hooks().shm__side_dump(self.h, None, None, 0, info), "side_dump")
        n = int(info[0]) if pages is None else int(pages)
        if n > info[1]:
            raise ValueError("side_dump: more pages than the arena has")
        lines = np.zeros((n, 64), dtype=np.uint8)
        hw = np.zeros(n, dtype=np.uint8)
        _check(_hooks().shm__side_dump(self.h, lines.ctypes.data_as(vp), hw.ctypes.data_as(vp),
                                       n, info), "side_dump")
        return lines, hw, {"next_page": int(info[0]), "cap_pages": int(info[1])}

    def vt_stats(self):
        """Test hook (shm__vt_stats): the key-value bucket table a read
        phase's gets read first: buckets, bytes, dead buckets, the stored keys
        that ended in dead buckets at the last build, the stored keys then,
        and whether gets and chunks use it (all 0 without a table)."""
        out = (u64 * 6)()
        _check(_hooks().shm__vt_stats(self.h, out), "vt_stats")
        return {"buckets": out[0], "bytes": out[1], "dead_buckets": out[2],
                "dead_keys_at_build": out[3], "keys_at_build": out[4], "trusted": bool(out[5])}

    def vt_dump(self):
        """Test hook (shm__vt_dump): the raw bucket table as an (n, 16)
        uint64 array (one 128 B bucket per row: key, value of slots 0..7;
        n == 0 without a table) and {"lo", "shift", "trusted"}: bucket b
        covers the keys [lo + (b << shift), lo + ((b + 1) << shift))."""
        import numpy as np
        info = (u64 * 4)()
        _check(_hooks().shm__vt_dump(self.h, None, 0, info), "vt_dump")
        b = np.zeros((int(info[0]), 16), dtype=np.uint64)
        if info[0]:
            _check(_hooks().shm__vt_dump(self.h, b.ctypes.data_as(vp), info[0], info), "vt_dump")
            assert info[0] == b.shape[0]
        return b, {"lo": int(info[1]), "shift": int(info[2]), "trusted": bool(info[3])}


def order_limits():
    """Test hook (shm__order_limits; no GPU): the compiled constants that
    decide the path an insert chunk's ordering takes (isort.hip)."""
    out = (u64 * 6)()
    _check(_hooks().shm__order_limits(out), "order_limits")
    names = ("tile", "max_tiles", "uniq_cap", "sub_cap", "coarse", "fine")
    return {k: int(v) for k, v in zip(names, out)}


def check_image(image, root_ptr, node=0):
    """Test hook (shm__check_image; no GPU): the structural check behind
    Tree.check() on a host image.  Returns (code, counts): the check's raw
    code (0 = sound) and {"leaves", "internal", "keys"} as it counted them
    (all 0 for a rejected image)."""
    import numpy as np
    image = np.ascontiguousarray(image, dtype=np.uint8)
    counts, code = (u64 * 3)(), ctypes.c_int(0)
    _check(_hooks().shm__check_image(image.ctypes.data_as(vp), image.nbytes,
                                     from_i64(int(root_ptr)), node, counts,
                                     ctypes.byref(code)), "check_image")
    return code.value, dict(leaves=counts[0], internal=counts[1], keys=counts[2])


class LocalGroup:
    """P in-process ranks on one GPU for CShard.local (test hook): every
    rank is driven by its own host thread, all on one shared stream."""

    def __init__(self, world):
        g = vp()
        _check(_hooks().shm__local_group_create(world, ctypes.byref(g)), "local_group")
        self.h, self.world = g, world

    def close(self):
        if getattr(self, "h", None):
            _hooks().shm__local_group_destroy(self.h)
            self.h = None
