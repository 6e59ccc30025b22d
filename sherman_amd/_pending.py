"""Results of the calls that queue work without a host wait."""
from ._abi import SHM_EIO, SHM_ENOSPC, ShermanError


class _StreamDone:
    """Completion of the work queued so far on a raw hipStream_t (None = the
    null stream) of `device`, for a pending result: .synchronize() waits for
    that stream.  No event is recorded at issue time -- a record between two
    kernels leaves the device idle ~5-7 us (tools/event_gap.hip) -- so the
    wait may also cover work queued there later, never less."""

    def __init__(self, stream_ptr, device):
        self.stream_ptr, self.device = stream_ptr, device

    def synchronize(self):
        import torch
        s = (torch.cuda.ExternalStream(self.stream_ptr, device=self.device) if self.stream_ptr
             else torch.cuda.default_stream(self.device))
        s.synchronize()


class PendingRange:
    """Result of Tree.range_query_batch_async: (counts, values) once the
    scans have run.  tot = device (total, error bits); done = the stream the
    scans were queued on (_StreamDone: resolved when they were issued, so
    .result() waits for them whatever stream is current then)."""

    def __init__(self, tree, counts, vals, tot=None, done=None):
        self.tree, self.counts, self.vals, self.tot, self.done = tree, counts, vals, tot, done

    def result(self):
        if self.tot is None:  # ran synchronously
            return self.counts, self.vals
        import torch
        if self.done is not None:
            self.done.synchronize()
        else:
            torch.cuda.synchronize()
        total, err = (int(x) for x in self.tot.cpu().tolist())
        if err:
            self.tree.synchronize()  # raises the device error
            raise ShermanError(SHM_EIO, "range_query_batch_async")
        # learn the size even when this batch overflowed, so the next async
        # batch gets a buffer that fits
        self.tree._rq_cap = max(self.tree._rq_cap, total + total // 4)
        if total > self.vals.numel():
            raise ShermanError(SHM_ENOSPC, "range_query_batch_async: %d values, buffer %d"
                               % (total, self.vals.numel()))
        self.tot = None
        self.vals = self.vals[:total]
        return self.counts, self.vals


class PendingSlots:
    """Result of Tree.range_query_slots: (counts, vals[n, slot_cap]) once the
    scans have run; .result() raises the device error, if any, and
    SHM_ENOSPC when some scan's count passed slot_cap (its buffer then holds
    its first slot_cap values)."""

    def __init__(self, tree, counts, vals, slot_cap, status, done):
        self.tree, self.counts, self.slot_cap = tree, counts, slot_cap
        self.vals = vals.view(-1)[:counts.numel() * slot_cap].view(counts.numel(), slot_cap)
        self.status, self.done = status, done

    def check(self):
        """Scans over slot_cap once the scans have run (device errors raise)."""
        if self.done is not None:
            self.done.synchronize()
        self.tree.synchronize()  # raises a device error of the queued calls
        return int((self.counts > self.slot_cap).sum().item())

    def result(self):
        ovf = self.check()
        if ovf:
            raise ShermanError(SHM_ENOSPC, "range_query_slots: %d scans passed slot_cap %d"
                               % (ovf, self.slot_cap))
        return self.counts, self.vals

    def packed(self):
        """(counts, values concatenated in scan order): the compact form."""
        import torch
        c, v = self.result()
        if c.numel() == 0:
            return c, v.view(-1)[:0]
        mask = torch.arange(self.slot_cap, device=c.device)[None, :] < c[:, None]
        return c, v[mask]


class PendingScan:
    """Result of Tree.scan_batch / Tree.rscan_batch: (counts, keys[n, limit],
    vals[n, limit]) once the scans have run.  Scan i's pairs, in the order of
    the call that made it (scan_batch: ascending unsigned key order,
    rscan_batch: descending), are keys[i, :counts[i]] and vals[i, :counts[i]]
    (int64 bit patterns of the u64 words); the rest of its row is whatever the
    buffers held.  counts[i] == limit means there may be more: keys[i, limit -
    1] + 1 is the next `lo` of a scan_batch, keys[i, limit - 1] - 1 the next
    `hi` of an rscan_batch (unless that key is 0)."""

    def __init__(self, tree, counts, keys, vals, limit, status, done):
        n = counts.numel()
        self.tree, self.counts, self.limit = tree, counts, limit
        self.keys = keys.view(-1)[:n * limit].view(n, limit)
        self.vals = vals.view(-1)[:n * limit].view(n, limit)
        self.status, self.done = status, done

    def check(self):
        """Waits for the scans; a device error of the queued calls raises."""
        if self.done is not None:
            self.done.synchronize()
        self.tree.synchronize()

    def result(self):
        self.check()
        return self.counts, self.keys, self.vals
