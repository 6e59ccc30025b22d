"""What recurs with the chunk counter and the scan counter: aged handles.

Device state is never reset and is told apart by tags derived from counters
(DESIGN.md "Counters and their periods").  When a tag recurs, a stale word
equals a fresh one unless a host-side clear prevents it.  These tests take a
handle to the chunks and scans where the tags recur -- by real streams for
the short periods (2 and 255 chunks), by the forward-only test hook
shm__seq_jump for the long ones (65,535 scans; 65,536, 2^29 and 2^32 chunks)
-- and compare it there with two references of the same operation:

* OracleTree (oracle/sherman_oracle.c), the CPU tree, for contents and every
  kind of read;
* a fresh twin: the aged tree's dump_image() loaded into a new handle, whose
  counters are near 0 and whose lock table, marks and tagged words are zero.
  The same chunks go to both; beyond the contents the twin pins the work the
  chunk did (profile_read's insert_unique / insert_dels / insert_staged: a
  stale page mark stages a page the twin does not) and the pages and splits
  it made.

Everything compared is integer state: equality, no tolerance.
"""
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, host, lib_ok, U64  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402
from rscan_model import RScanModel  # noqa: E402
from scan_model import ScanModel  # noqa: E402

KEY_MAX = (1 << 64) - 1
ERR_KEYMAX = 1 << 31  # kernels.h kErrKeyMax
ARENA = 64 << 20
MAX_BATCH = 1 << 10

# The key universe: N_BASE stored "anchor" keys spread over the key space (so
# the leaf directory's prefixes tell them apart), cluster i = the keys just
# above anchor i.  About 36 to 54 neighbouring anchors share a leaf.
N_BASE = 4000
SHIFT = 50


def anchor(i):
    return (np.asarray(i, dtype=U64) + U64(1)) << U64(SHIFT)


# ---- chunks -----------------------------------------------------------------
class Stream:
    """Chunks of mixed traffic over the clusters outside `quiet` (anchor
    indices no random op may touch, nor their leaf neighbours): overwrites of
    anchors, new keys, deletes of earlier new keys (value 0), the same key
    twice in a chunk.  The stored key count stays within 3,000 .. 6,000."""

    def __init__(self, seed, quiet=()):
        self.rng = np.random.default_rng(seed)
        ok = np.ones(N_BASE, dtype=bool)
        for q in quiet:
            ok[max(0, q - 60):q + 61] = False
        self.free = np.flatnonzero(ok)
        self.extras = []  # new keys stored so far (delete candidates)
        self.serial = 0   # makes every new key distinct

    def new_keys(self, cluster, n):
        k = anchor(cluster) + U64(1) + np.arange(self.serial, self.serial + n, dtype=U64)
        self.serial += n
        return k

    def vals(self, n):
        return self.rng.integers(1, 1 << 62, n).astype(U64)

    def mixed(self, n):
        rng = self.rng
        n_new = n // 8
        n_del = min(n // 8, len(self.extras))
        n_dup = n // 16
        n_over = n - n_new - n_del - n_dup
        parts_k, parts_v = [], []
        over = anchor(rng.choice(self.free, n_over))
        parts_k.append(over)
        parts_v.append(self.vals(n_over))
        if n_new:
            cl = rng.choice(self.free, n_new)
            nk = np.concatenate([self.new_keys(c, 1) for c in cl])
            parts_k.append(nk)
            parts_v.append(self.vals(n_new))
        # in-batch duplicates: upserts of this chunk again, later in batch
        # order, with another value (the last writer wins)
        allk = np.concatenate(parts_k)
        dup = allk[rng.integers(0, allk.size, n_dup)]
        if n_del:
            idx = sorted(rng.choice(len(self.extras), n_del, replace=False).tolist(), reverse=True)
            dk = np.array([self.extras.pop(j) for j in idx], dtype=U64)
            parts_k.append(dk)
            parts_v.append(np.zeros(n_del, dtype=U64))
        if n_new:
            self.extras.extend(nk.tolist())
        k, v = np.concatenate(parts_k), np.concatenate(parts_v)
        p = rng.permutation(k.size)
        return np.concatenate([k[p], dup]), np.concatenate([v[p], self.vals(n_dup)])

    def overwrites(self, n):
        """A quick-path chunk: stored anchors only, no new key, no delete."""
        return anchor(self.rng.choice(self.free, n)), self.vals(n)

    def burst(self, cluster, n):
        """n new keys for one leaf: more than kSmallSplit pages' worth."""
        return self.new_keys(cluster, n), self.vals(n)

    def rejected(self, n):
        k, v = self.overwrites(n)
        k[n // 2] = U64(KEY_MAX)
        return k, v


class Chunk:
    def __init__(self, k, v, rejected=False):
        assert 0 < k.size == v.size <= MAX_BATCH
        self.kh, self.vh = k.astype(U64), v.astype(U64)
        self.k, self.v = dev(self.kh), dev(self.vh)
        self.rejected = rejected


# ---- the three trees ----------------------------------------------------------
def make_tree(leaf_dir=True, max_batch=MAX_BATCH):
    return shm.Tree(arena_bytes=ARENA, max_batch=max_batch, leaf_dir=leaf_dir)


def load_base(t, orc, rng):
    k = anchor(np.arange(N_BASE))
    v = rng.integers(1, 1 << 62, N_BASE).astype(U64)
    p = rng.permutation(N_BASE)
    t.insert_batch(dev(k[p]), dev(v[p]))
    orc.apply_batch(k[p], v[p])


def twin_of(t, leaf_dir=True):
    """The aged tree's image in a fresh handle."""
    img, root = t.dump_image()
    tw = make_tree(leaf_dir, t.max_batch)
    tw.load_image(img, root)
    return tw


def expect_status(call, rejected):
    """Run a synchronising call; a rejected chunk before it shows as
    SHM_EINVAL with exactly the KEY_MAX bit, anything else as no error."""
    try:
        call()
        got = 0
    except shm.ShermanError as e:
        got = e.rc
    assert got == (shm.SHM_EINVAL if rejected else 0)


def settle_error(t, rejected):
    e = t.last_error(reset=True)
    assert e["bits"] == (ERR_KEYMAX if rejected else 0), hex(e["bits"])
    if rejected:
        assert e["status"] == shm.SHM_EINVAL


class Pipe:
    """The two-stream pipeline of tests/test_gpu_progress.py: chunk i + 1 is
    ordered on one stream while chunk i applies on another.  SHM_EAGAIN from
    insert_order (two tickets out, or the chunk ids starting over) is answered
    by applying the oldest ticket and ordering again."""

    def __init__(self, t):
        self.t = t
        self.s_ord, self.s_app = torch.cuda.Stream(), torch.cuda.Stream()
        self.tickets = []
        self.eagain = 0
        self.keep = []

    def _apply_oldest(self, after=None):
        self.t.insert_apply(self.tickets.pop(0), stream=self.s_app)
        if after:
            after(self.s_app)

    def run(self, chunks, after=None):
        torch.cuda.synchronize()  # the chunks' tensors exist
        self.keep = list(chunks)
        for c in chunks:
            try:
                tk = self.t.insert_order(c.k, c.v, stream=self.s_ord)
            except shm.ShermanError as e:
                assert e.rc == shm.SHM_EAGAIN and self.tickets
                self.eagain += 1
                self._apply_oldest(after)
                tk = self.t.insert_order(c.k, c.v, stream=self.s_ord)
            self.tickets.append(tk)
            if len(self.tickets) == 2:
                self._apply_oldest(after)
        while self.tickets:
            self._apply_oldest(after)


def apply_chunks(t, chunks, mode, pipe=None, after=None):
    """The chunks on tree t: one insert_batch each ("batch") or all of them
    through the pipeline ("pipe"), then the status."""
    rej = any(c.rejected for c in chunks)
    if mode == "batch":
        for c in chunks:
            expect_status(lambda: t.insert_batch(c.k, c.v), c.rejected)
            settle_error(t, c.rejected)
            if after:
                after(None)
    else:
        pipe.run(chunks, after)
        expect_status(t.synchronize, rej)
        settle_error(t, rej)


def oracle_apply(orc, chunks):
    for c in chunks:
        if not c.rejected:  # rejected whole: nothing of it is applied
            orc.apply_batch(c.kh, c.vh)


def by_range(counts, vals):
    """(range, value) pairs sorted: equal for two scans' outputs exactly when
    every range's values are the same set at the place its offset gives."""
    rid = np.repeat(np.arange(counts.size), counts.astype(np.int64))
    o = np.lexsort((vals, rid))
    return rid[o], vals[o]


def compare_reads(t, orc, rng):
    """Every kind of read on t against the oracle and the scan models."""
    ok, ov = orc.dump()
    o = np.argsort(ok, kind="stable")
    ok, ov = ok[o], ov[o]
    n = ok.size
    assert 3000 <= n <= 6000, n
    ek, ev = t.export()
    assert np.array_equal(host(ek), ok) and np.array_equal(host(ev), ov), "export differs"
    assert t.count() == n
    assert t.check()["keys"] == n
    assert orc.check()[0] == 0
    # gets of every stored key, and misses beside them
    probe = np.concatenate([ok, ok[rng.integers(0, n, 512)] + U64(1 << (SHIFT - 1)) + U64(3)])
    wv, wf = orc.search_batch(probe)
    assert not wf[n:].any()
    pk = dev(probe)
    gv = torch.empty_like(pk)
    gf = torch.empty(pk.numel(), dtype=torch.uint8, device="cuda")
    t.search_batch(pk, gv, gf)
    t.synchronize()
    assert np.array_equal(gf.cpu().numpy(), wf), "found flags differ"
    assert np.array_equal(host(gv)[wf != 0], wv[wf != 0]), "values differ"
    # ordered scans both ways
    fwd, rev = ScanModel(ok, ov), RScanModel(ok, ov)
    lo = np.sort(ok[rng.integers(0, n, 48)] - U64(1))
    c, k, v = t.scan_batch(dev(lo), 8).result()
    mc, mk, mv, mw = fwd.scan(lo, 8)
    assert np.array_equal(c.cpu().numpy(), mc)
    assert np.array_equal(host(k).reshape(-1, 8)[mw], mk[mw])
    assert np.array_equal(host(v).reshape(-1, 8)[mw], mv[mw])
    c, k, v = t.rscan_batch(dev(lo), 8).result()
    mc, mk, mv, mw = rev.scan(lo, 8)
    assert np.array_equal(c.cpu().numpy(), mc)
    assert np.array_equal(host(k).reshape(-1, 8)[mw], mk[mw])
    assert np.array_equal(host(v).reshape(-1, 8)[mw], mv[mw])
    # inclusive range scans
    hi = lo + U64(12 << SHIFT)
    c, v = t.range_query_batch(dev(lo), dev(hi))
    oc, ovv = orc.range_query_batch(lo, hi)
    a, b = fwd.bounds(lo, hi)
    assert np.array_equal(host(c), oc) and np.array_equal(oc.astype(np.int64), b - a)
    g, w = by_range(host(c), host(v)), by_range(oc, ovv)
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
    t.synchronize()
    assert t.last_error()["bits"] == 0


def compare_twin(t, tw, chunks, orc, rng, mode, pipe=None, after=None):
    """The same chunks on the aged tree (by `mode`) and on its twin (one
    insert_batch each): the work they did, the pages and splits they made,
    and then every read of both against the oracle."""
    before = [x.stats() for x in (t, tw)]
    for x in (t, tw):
        x.profile(True)
        x.profile_read(reset=True)
    apply_chunks(t, chunks, mode, pipe, after)
    apply_chunks(tw, chunks, "batch")
    prof = [x.profile_read(reset=True) for x in (t, tw)]
    for x in (t, tw):
        x.profile(False)
    oracle_apply(orc, chunks)
    for f in ("insert_unique", "insert_dels", "insert_staged"):
        assert prof[0][f] == prof[1][f], (f, prof[0][f], prof[1][f])
    st = [x.stats() for x in (t, tw)]
    assert st[0]["pages_used"] == st[1]["pages_used"]
    # the twin's split count starts at 0: what the chunks added
    assert st[0]["splits"] - before[0]["splits"] == st[1]["splits"] - before[1]["splits"]
    compare_reads(t, orc, rng)
    compare_reads(tw, orc, rng)
    return prof[0]


def searcher(t, probe):
    """Between chunks: a small search, so a tree with a leaf directory is in
    the state where the chunks keep it (dir upkeep after every k_upper)."""
    out = torch.empty_like(probe)

    def after(stream):
        t.search_batch(probe, out, None, stream=stream)
    return after


# ---- A. real streams: the periods 2 and 255 -------------------------------------
# (T, cluster that gets a new key in chunk T and only overwrites in chunk
# T + 255, cluster with the two the other way round).  The pairs lie on both
# sides of the chunks 255 and 510, whose tags are multiples of 255; T = 255
# itself brings its clusters' new keys under the tag whose mark is 1.
A_PAIRS = [(6, 100, 350), (100, 600, 850), (254, 1100, 1350), (255, 1600, 1850),
           (256, 2100, 2350), (300, 2600, 2850), (345, 3100, 3350)]
A_CHUNKS = 600


def a_schedule():
    sched = {}
    for T, c1, c2 in A_PAIRS:
        sched.setdefault(T, []).append((c1, "new"))
        sched.setdefault(T, []).append((c2, "over"))
        sched.setdefault(T + 255, []).append((c1, "over"))
        sched.setdefault(T + 255, []).append((c2, "new"))
    return sched


@pytest.mark.parametrize("leaf_dir", [True, False], ids=["dir", "nodir"])
@pytest.mark.parametrize("mode", ["batch", "pipe"])
def test_a_real_stream_across_mark_periods(lib_ok, mode, leaf_dir):
    """600 chunks on one handle.  A leaf that got a new key in chunk T carries
    the byte mark new_mark(T) (kernels.h); chunk T + 255 has the same mark
    and brings that leaf overwrites only, so with the marks' clear missing
    (tree_insert.cpp insert_apply, new_mark(tag) == 1) the leaf is staged again:
    insert_staged above the twin's.  Contents against the oracle every 50
    chunks and at the end."""
    t0 = time.perf_counter()
    rng = np.random.default_rng(1)
    quiet = [c for _, c1, c2 in A_PAIRS for c in (c1, c2)]
    st = Stream(2, quiet)
    t, orc = make_tree(leaf_dir), OracleTree(ARENA)
    load_base(t, orc, rng)
    pipe = Pipe(t) if mode == "pipe" else None
    after = searcher(t, dev(anchor(rng.integers(0, N_BASE, 64)))) if leaf_dir else None
    sched = a_schedule()
    watched_new = {}  # cluster -> the keys it got

    def chunk_for(tag):
        k, v = st.mixed(int(st.rng.integers(64, 200)))
        for c, kind in sched.get(tag, ()):
            if kind == "new":
                nk = st.new_keys(c, 2)
                watched_new[c] = nk
                k, v = np.concatenate([k, nk]), np.concatenate([v, st.vals(2)])
            else:  # stored keys of the leaf only: its anchors, and the keys it got in chunk T
                ow = np.concatenate([anchor(np.arange(c - 2, c + 3)), watched_new.get(c, anchor([c]))])
                k, v = np.concatenate([k, ow]), np.concatenate([v, st.vals(ow.size)])
        assert k.size <= 256
        return Chunk(k, v)

    tag = t.last_chunk()
    stops = sorted({T + 255 for T, _, _ in A_PAIRS} | set(range(50, A_CHUNKS + 1, 50)) | {A_CHUNKS})
    for stop in stops:
        twin_stop = stop - 255 in {T for T, _, _ in A_PAIRS}
        last = stop - 1 if twin_stop else stop
        seg = [chunk_for(x) for x in range(tag + 1, last + 1)]
        if seg:
            apply_chunks(t, seg, mode, pipe, after)
            oracle_apply(orc, seg)
        if twin_stop:
            tw = twin_of(t, leaf_dir)
            compare_twin(t, tw, [chunk_for(stop)], orc, rng, mode, pipe, after)
            tw.close()
        elif stop % 50 == 0:
            compare_reads(t, orc, rng)
        tag = stop
        assert t.last_chunk() == tag
    compare_reads(t, orc, rng)
    orc.close()
    t.close()
    print(f"scenario A {mode} {'dir' if leaf_dir else 'nodir'}: {time.perf_counter() - t0:.2f} s")


# ---- B. the scans' 16-bit tags ---------------------------------------------------
def range_scan(t, lo, hi, cap):
    """shm_range_query_batch with its offsets: (counts, offsets, values, total)."""
    n = lo.numel()
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    offs = torch.empty(n, dtype=torch.int64, device="cuda")
    vals = torch.empty(cap, dtype=torch.int64, device="cuda")
    total = ctypes.c_uint64(0)
    rc = shm.lib().shm_range_query_batch(t.h, shm._ptr(lo), shm._ptr(hi), n, shm._ptr(counts),
                                         shm._ptr(offs), shm._ptr(vals), cap, ctypes.byref(total),
                                         None)
    assert rc == 0, rc
    t.synchronize()
    return host(counts), host(offs), host(vals)[:total.value], int(total.value)


def scan_seq_is(t, value):
    """Pins the scan counter with the hook's own rule: a jump to the counter
    changes nothing, a jump below it is refused."""
    t.seq_jump("scan", value)
    with pytest.raises(shm.ShermanError) as e:
        t.seq_jump("scan", value - 1)
    assert e.value.rc == shm.SHM_EINVAL


def test_b_scan_tags_recur_after_the_wrap(lib_ok):
    """launch_scan_u64_total's tile words carry scan_seq & 0xFFFF; scan_tag
    (tree_read.cpp) zeroes them when the tag wraps and skips tag 0.  A three-tile
    scan P leaves its tile sums under tag 0xFFFB; single-tile scans cross the
    wrap (they rewrite word 0 only); then a three-tile scan Q runs under the
    same 16-bit tag, 65,536 counter steps later.  With the clear missing,
    Q's later tiles could take P's sums for Q's: Q's offsets must be the
    exact prefix sums of its counts.  Only shm_range_query_batch (and its
    async form and the shard router's scan) use these words: scan_batch,
    rscan_batch and export have scan-free or own workspaces."""
    rng = np.random.default_rng(3)
    t, orc = make_tree(True, 1 << 12), OracleTree(ARENA)
    load_base(t, orc, rng)
    ok, ov = orc.dump()
    model = ScanModel(ok, ov)
    n = 3000  # three kSegTile tiles in one launch (max_batch 4096)

    def ranges(pattern):
        a = rng.integers(0, N_BASE - 16, n)
        lo = model.keys[a] + np.where(pattern == 0, U64(1), U64(0))
        hi = np.where(pattern == 0, lo, model.keys[a + np.maximum(pattern, 1) - 1])
        return lo, hi

    def big(pattern):
        lo, hi = ranges(pattern)
        c, o, v, total = range_scan(t, dev(lo), dev(hi), 1 << 16)
        assert np.array_equal(c.astype(np.int64), pattern)
        assert np.array_equal(o.astype(np.int64), np.cumsum(pattern) - pattern), "offsets"
        assert total == int(pattern.sum())
        oc, ovv = orc.range_query_batch(lo, hi)
        assert np.array_equal(oc, c)
        a, b = model.bounds(lo, hi)
        want = np.concatenate([model.vals[x:y] for x, y in zip(a, b)])
        g, w = by_range(c, v), by_range(oc, ovv)
        assert np.array_equal(g[1], w[1]) and np.array_equal(np.sort(want), np.sort(v))

    def small():
        lo = np.sort(model.keys[rng.integers(0, N_BASE - 16, 64)])
        hi = lo + U64(3 << SHIFT)
        c, o, v, total = range_scan(t, dev(lo), dev(hi), 1 << 12)
        a, b = model.bounds(lo, hi)
        assert np.array_equal(c.astype(np.int64), b - a) and total == int((b - a).sum())
        assert np.array_equal(o.astype(np.int64), np.cumsum(b - a) - (b - a))

    P = (np.arange(n) * 7 % 5).astype(np.int64)
    Q = ((np.arange(n) * 3 + 1) % 7).astype(np.int64)
    t.seq_jump("scan", 0xFFFA)
    big(P)                         # scan_seq 0xFFFB: tag 0xFFFB
    for _ in range(12):            # 0xFFFC .. 0xFFFF, the wrap (0x10000 stepped over), .. 0x10008
        small()
    scan_seq_is(t, 0x10008)
    t.seq_jump("scan", 0xFFFB + 0x10000 - 1)
    big(Q)                         # scan_seq 0x1FFFB: tag 0xFFFB again
    scan_seq_is(t, 0x1FFFB)
    # a large scan whose own tag is the one after the wrap
    t.seq_jump("scan", 0x1FFFF)
    big(P)                         # 0x20000 is tag 0: cleared, stepped over; the scan runs as tag 1
    scan_seq_is(t, 0x20001)
    big(Q)
    # a jump that lands on a multiple of 2^16 rests behind it, as scan_tag does
    t.seq_jump("scan", 0x30000)
    scan_seq_is(t, 0x30001)
    big(P)
    # the end of the 32-bit counter: 2^32 is a multiple of 2^16 like any other
    t.seq_jump("scan", 0xFFFFFFFE)
    big(Q)                         # 0xFFFFFFFF
    big(P)                         # 0 -> cleared -> 1
    scan_seq_is(t, 1)
    big(Q)
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


# ---- C. the ordering's 16-bit chunk tags --------------------------------------------
def c_phase(t, orc, st, rng, first_tag):
    """40 real chunks from first_tag on, of varying size (so the 256 bins hold
    other counts each time), one of them rejected and directly followed by a
    normal one; the twin gets the same."""
    assert t.last_chunk() == first_tag - 1
    tw = twin_of(t)
    sizes = st.rng.integers(64, 513, 40)
    for i in range(0, 40, 5):
        seg = []
        for j in range(i, i + 5):
            if j == 21:
                seg.append(Chunk(*st.rejected(int(sizes[j])), rejected=True))
            else:
                seg.append(Chunk(*st.mixed(int(sizes[j]))))
        for c in seg:  # chunk by chunk: the work of each against the twin's
            compare_twin_light(t, tw, c)
        oracle_apply(orc, seg)
        compare_reads(t, orc, rng)
        compare_reads(tw, orc, rng)
        assert t.last_chunk() == first_tag + i + 4
    tw.close()


def compare_twin_light(t, tw, c):
    """One chunk on both trees: status, error bits, its counts, pages, splits."""
    d = []
    for x in (t, tw):
        s0 = x.stats()
        x.profile(True)
        x.profile_read(reset=True)
        apply_chunks(x, [c], "batch")
        p = x.profile_read(reset=True)
        x.profile(False)
        s1 = x.stats()
        d.append((p["insert_unique"], p["insert_dels"], p["insert_staged"], s1["pages_used"],
                  s1["splits"] - s0["splits"]))
    assert d[0] == d[1], d
    if c.rejected:
        assert d[0][:3] == (0, 0, 0)


def test_c_bin_tags_recur_after_65536_chunks(lib_ok):
    """k_bin_unique's look-back words carry tag & 0xFFFF (isort.hip
    bin_prefix) and are never cleared: a launch is safe because every launch
    that is not rejected publishes all 256 words under its own tag before it
    reads any (both paths of every block call bin_prefix), so the words a
    launch finds are those of the last launch that was not rejected, one tag
    back.  A rejected chunk returns before bin_prefix: the words keep the tag
    of the chunk before it, which the next chunk cannot have either.  The 40
    chunks run across 0x10000 and again 65,536 tags later, where the tags of
    the first run recur."""
    rng = np.random.default_rng(5)
    st = Stream(6)
    t, orc = make_tree(), OracleTree(ARENA)
    load_base(t, orc, rng)
    t.seq_jump("chunk", 0xFFF0)
    assert t.last_chunk() == 0xFFF0
    c_phase(t, orc, st, rng, 0xFFF1)
    assert t.last_chunk() == 0x10018
    t.seq_jump("chunk", 0x1FFF0)
    assert t.last_chunk() == 0x1FFF0
    c_phase(t, orc, st, rng, 0x1FFF1)
    # the hook refuses to go back, and to move while a ticket is out
    with pytest.raises(shm.ShermanError):
        t.seq_jump("chunk", 0x1FFF0)
    c = Chunk(*st.overwrites(64))
    tk = t.insert_order(c.k, c.v)
    with pytest.raises(shm.ShermanError):
        t.seq_jump("chunk", 0x30000)
    t.insert_apply(tk)
    t.synchronize()
    oracle_apply(orc, [c])
    compare_reads(t, orc, rng)
    orc.close()
    t.close()


# ---- D. the fan-in tags: 2^29 chunks -------------------------------------------------
def test_d_fan_tags_recur_after_2_pow_29_chunks(lib_ok):
    """A leaf that gets about 300 new keys in one chunk splits into more than
    kSmallSplit pages: its sibling builders count themselves into the
    segment's word leaf_rd[g] under fan_tag = (uint32_t)(chunk << 3) | level
    (split_wave.h) and the builder of page 0 waits for (tag, P - 1).  At chunk
    X + 2^29 the same word meets the same tag: left as (tag, 8) it would
    make fan_arrive count on from 8 -- fan_in would pass at once for the same
    P (page 0 rewritten under its readers) or never for another P
    (kErrFanIn).  insert_apply clears the words at the chunk whose tag has
    zero low 29 bits; that chunk runs for real here (tag 2^29), the one at
    2^30 is crossed by the hook, which makes the same clear."""
    rng = np.random.default_rng(7)
    st = Stream(8, quiet=[500, 1500, 2500])
    t, orc = make_tree(), OracleTree(ARENA)
    load_base(t, orc, rng)
    X = t.last_chunk() + 1

    def big_split(cluster, n):
        tw = twin_of(t)
        s0 = t.stats()["pages_used"]
        p = compare_twin(t, tw, [Chunk(*st.burst(cluster, n))], orc, rng, "batch")
        tw.close()
        assert p["insert_staged"] == 1  # one segment: the word is leaf_rd[0] each time
        return t.stats()["pages_used"] - s0

    # about 45 stored keys + 300 at 36 per page: 10 pages; + 150: 5 or 6
    np1 = big_split(500, 300)
    assert t.last_chunk() == X and np1 >= 8, np1
    t.seq_jump("chunk", (1 << 29) - 1)
    tw = twin_of(t)
    compare_twin(t, tw, [Chunk(*st.mixed(128))], orc, rng, "batch")  # tag 2^29: the clear
    tw.close()
    assert t.last_chunk() == 1 << 29
    t.seq_jump("chunk", X + (1 << 29) - 1)
    np2 = big_split(1500, 300)  # the same shape under the same fan tag
    assert t.last_chunk() == X + (1 << 29) and np2 >= 8, np2
    t.seq_jump("chunk", X + (1 << 30) - 1)
    np3 = big_split(2500, 150)  # another page count, the tag a third time
    assert t.last_chunk() == X + (1 << 30) and 4 <= np3 < 8, np3
    orc.close()
    t.close()


# ---- E. the end of the counter: 2^32 ---------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "pipe"])
def test_e_handle_crosses_the_end_of_the_chunk_counter(lib_ok, mode):
    """40 chunks from tag 2^32 - 19 on: the chunk after 2^32 - 1 is tag 1 of a
    new epoch (tree_insert.cpp epoch_reset: the handle drained, the lock table and
    every tagged word zeroed, the mirrors reset).  Without it every lock word
    an old chunk touched stays above tag << 32 of the new tags (kErrLock
    after the spin bound) and gate, skip and the tagged words of the handle's
    first chunks could equal a new tag.  Contents, statuses, error bits and
    the work of every chunk equal the twin's and the oracle's before, at and
    after the crossing; reads of every kind lie between."""
    rng = np.random.default_rng(9)
    st = Stream(10, quiet=[700, 2200])
    t, orc = make_tree(), OracleTree(ARENA)
    load_base(t, orc, rng)
    # the handle's first chunks leave gate and skip at small tags: a rejected
    # chunk (gate = 5) and a quick-path chunk (skip[0] = 6), tags that return
    first = [Chunk(*st.rejected(64), rejected=True), Chunk(*st.overwrites(64))]
    apply_chunks(t, first, "batch")
    oracle_apply(orc, first)
    assert t.last_chunk() == 6
    start = (1 << 32) - 20
    t.seq_jump("chunk", start)
    assert t.last_chunk() == start
    pipe = Pipe(t) if mode == "pipe" else None
    tw = twin_of(t)
    # chunk i has tag start + 1 + i up to i = 18 (2^32 - 1), then i - 18: the
    # tags 5 and 6 return at i = 23 and 24, which bring new keys and deletes
    # (a stale gate would drop the first whole, a stale skip the splits and
    # deletes of the second)
    kinds = {3: "burst", 9: "quick", 14: "rej", 26: "quick", 28: "burst", 33: "rej"}
    want_tag = start

    def make(i):
        kind = kinds.get(i, "mixed")
        n = int(st.rng.integers(64, 513))
        if kind == "burst":
            return Chunk(*st.burst(700 if i == 3 else 2200, 300))
        if kind == "quick":
            return Chunk(*st.overwrites(n))
        if kind == "rej":
            return Chunk(*st.rejected(n), rejected=True)
        return Chunk(*st.mixed(n))

    for i in range(0, 40, 4):
        seg = [make(j) for j in range(i, i + 4)]
        if mode == "batch":
            for c in seg:
                compare_twin_light(t, tw, c)
        else:
            apply_chunks(t, seg, "pipe", pipe)
            apply_chunks(tw, seg, "batch")
            assert t.stats()["pages_used"] == tw.stats()["pages_used"]
        oracle_apply(orc, seg)
        for _ in seg:
            want_tag = 1 if want_tag == (1 << 32) - 1 else want_tag + 1
        assert t.last_chunk() == want_tag  # 2^32 - 1 is followed by 1, never 0
        compare_reads(t, orc, rng)
        compare_reads(tw, orc, rng)
    assert t.last_chunk() == 21
    if mode == "pipe":
        assert pipe.eagain == 1  # once: the ticket of the old epoch applied first
    # the lock words' tag comes from the same counter
    t.lock_bench(dev(anchor(np.arange(N_BASE))))
    t.synchronize()
    assert t.last_error()["bits"] == 0
    tw.close()
    orc.close()
    t.close()
