"""Forward progress and completion order of the insert chain (round 5).

* the segmentation's look-back (k_seg_fill, seg_tile.h): a tile that waits
  too long for an earlier tile's word counts that tile's staged heads itself,
  so the list never depends on another block being placed (VERDICT r4 #6,
  ADVICE r4 medium).  Forced on every tile (shm__upper_force bit 3) the list
  must be the same: oracle contents;
* a C5-shaped chunk stream (new keys with small splits, deletes, range scans
  between) while another process holds 240 of the 256 CUs;
* k_upper's quick path (no split left to it, no delete): block 0 publishes
  the op buffers free while other blocks may not have started, so no block
  reads the ordering's delete count -- they read the segmentation kernel's
  copy (UpperCtl.ndel) -- and a pipelined ordering of chunk tag + 2 with
  deletes cannot be read by a late block of chunk tag.

Reference: every wait in the reference is on a lock a running thread holds
(src/Tree.cpp:205-242); batch semantics as in SURVEY §8a.
"""
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, host, lib_ok, U64  # noqa: E402
from oracle.pyoracle import OracleTree, to_key  # noqa: E402


HOG_SRC = r"""
import ctypes, sys, time
L = ctypes.CDLL(sys.argv[1])
L.shm__hog.restype = ctypes.c_int
L.shm__hog.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p]
hip = ctypes.CDLL("libamdhip64.so")
hip.hipDeviceSynchronize()
assert L.shm__hog(int(sys.argv[3]), int(sys.argv[2]), None) == 0
time.sleep(0.5)
print("started", flush=True)
assert hip.hipDeviceSynchronize() == 0
print("done", flush=True)
"""


def keys_of(t, lo, hi):
    """key(i) for i in [lo, hi) on the device (device CityHash = oracle
    to_key: tests/test_gpu_parity.py::test_device_cityhash_matches_oracle)."""
    k = torch.empty(hi - lo, dtype=torch.int64, device="cuda")
    t.gen_keys(lo, hi - lo, k)
    return k


def compare_contents(t, orc):
    ok, ov = orc.dump()
    dk = dev(ok)
    v = torch.empty_like(dk)
    f = torch.empty(dk.numel(), dtype=torch.uint8, device="cuda")
    t.search_batch(dk, v, f)
    t.synchronize()
    assert bool(f.all()), f"{int((f == 0).sum())} oracle keys missing on GPU"
    assert np.array_equal(host(v), ov)
    assert t.check()["keys"] == ok.size


def start_hog(ticks, blocks=240):
    proc = subprocess.Popen([sys.executable, "-c", HOG_SRC, shm.LIB_PATH, str(ticks), str(blocks)],
                            stdout=subprocess.PIPE, text=True)
    assert proc.stdout.readline().strip() == "started"
    return proc


def test_segmentation_tiles_count_late_tiles_themselves(lib_ok):
    """Every tile of every chunk counts its predecessors' staged heads
    itself (the fallback a tile takes after a bounded wait): chunks of new
    keys spread over many 1024-op tiles, updates and deletes, then contents
    equal to the oracle's and no error bit."""
    H = shm._hooks()
    t = shm.Tree(arena_bytes=512 << 20, max_batch=1 << 17)
    orc = OracleTree(512 << 20)
    base = keys_of(t, 1, 100001)
    t.insert_batch(base, base ^ 5)
    orc.apply_batch(host(base), host(base) ^ U64(5))
    rng = np.random.default_rng(5)
    for r in range(4):
        new = keys_of(t, 200001 + r * 30000, 230001 + r * 30000)
        old = base[torch.from_numpy(rng.integers(0, base.numel(), 40000)).cuda()]
        k = torch.cat([new, old])
        v = torch.from_numpy(rng.integers(1, 1 << 62, k.numel())).cuda()
        v[torch.from_numpy(rng.random(k.numel()) < 0.05).cuda()] = 0  # deletes
        assert H.shm__upper_force(t.h, 8) == 0
        t.insert_batch(k, v)
        orc.apply_batch(host(k), host(v))
    assert t.last_error()["bits"] == 0
    compare_contents(t, orc)
    assert orc.check()[0] == 0
    orc.close()
    t.close()


def test_c5_chunks_beside_cu_hog(lib_ok):
    """C5's shape beside another process that holds 240 CUs for 4 s: async
    insert chunks of new keys (small splits: early, in the upsert kernel),
    updates and deletes, a range scan after each, all queued without a host
    wait.  Every kernel of the chain (ordering bin prefix, segmentation
    look-back, upsert's block queue, k_upper) finishes on the CUs left, the
    scans and contents equal the oracle's, no error bit."""
    t = shm.Tree(arena_bytes=512 << 20, max_batch=1 << 17)
    orc = OracleTree(512 << 20)
    base = keys_of(t, 1, 200001)
    t.insert_batch(base, base ^ 3)
    orc.apply_batch(host(base), host(base) ^ U64(3))
    rng = np.random.default_rng(9)
    batches = []
    for r in range(5):
        new = keys_of(t, 300001 + r * 8000, 308001 + r * 8000)
        old = base[torch.from_numpy(rng.integers(0, base.numel(), 60000)).cuda()]
        k = torch.cat([new, old])
        v = torch.from_numpy(rng.integers(1, 1 << 62, k.numel())).cuda()
        v[torch.from_numpy(rng.random(k.numel()) < 0.03).cuda()] = 0
        batches.append((k, v))
    lo_h = np.sort(rng.integers(0, 1 << 63, 64, dtype=np.int64).astype(U64))
    hi_h = lo_h + U64(1 << 52)
    lo, hi = dev(lo_h), dev(hi_h)
    t.range_query_batch(lo, hi)  # sizes the async scan buffer
    torch.cuda.synchronize()
    proc = start_hog(400_000_000)
    try:
        pend = []
        for k, v in batches:
            t.insert_batch_async(k, v)
            pend.append(t.range_query_batch_async(lo, hi))
        res = [p.result() for p in pend]
        t.synchronize()
        assert proc.poll() is None, "the chunks outlasted the CU hog"
    finally:
        proc.wait(timeout=60)
    assert proc.returncode == 0
    for (k, v), (counts, vals) in zip(batches, res):
        orc.apply_batch(host(k), host(v))
        oc, ov = orc.range_query_batch(lo_h, hi_h)
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), np.asarray(oc, dtype=np.int64))
        assert np.array_equal(np.sort(host(vals)), np.sort(ov))
    assert t.last_error()["bits"] == 0
    compare_contents(t, orc)
    orc.close()
    t.close()


def test_quick_path_late_blocks_read_their_own_delete_count(lib_ok):
    """Pipelined chunks (shm_insert_order on one stream, shm_insert_apply on
    another) that alternate quick-path chunks -- new keys into leaves with
    room or small early splits, no delete, so k_upper only completes them --
    with delete-heavy chunks of the same buffer parity two tickets later,
    while a hog process delays the placement of k_upper's blocks.  A late
    block that read chunk tag + 2's delete count would apply its deletes
    early or from the wrong list: the contents after every applied chunk's
    searches, and at the end, equal the oracle's."""
    t = shm.Tree(arena_bytes=512 << 20, max_batch=1 << 16)
    orc = OracleTree(512 << 20)
    base = keys_of(t, 1, 120001)
    t.insert_batch(base, base ^ 7)
    orc.apply_batch(host(base), host(base) ^ U64(7))
    rng = np.random.default_rng(13)
    batches = []
    nxt = 500001
    for r in range(12):
        if r % 4 < 2:  # quick-path chunks: a few new keys, updates, no delete
            new = keys_of(t, nxt, nxt + 600)
            nxt += 600
            old = base[torch.from_numpy(rng.integers(0, base.numel(), 30000)).cuda()]
            k = torch.cat([new, old])
            v = torch.from_numpy(rng.integers(1, 1 << 62, k.numel())).cuda()
        else:  # deletes of stored keys (and some updates)
            k = base[torch.from_numpy(rng.integers(0, base.numel(), 20000)).cuda()]
            v = torch.from_numpy(rng.integers(1, 1 << 62, k.numel())).cuda()
            v[torch.from_numpy(rng.random(k.numel()) < 0.5).cuda()] = 0
        batches.append((k, v))
    s_ord, s_app = torch.cuda.Stream(), torch.cuda.Stream()
    s_ord.wait_stream(torch.cuda.current_stream())
    s_app.wait_stream(torch.cuda.current_stream())
    probe_h = host(base)[:20000]
    probe = dev(probe_h)
    outs = []
    proc = start_hog(300_000_000, blocks=252)
    try:
        tickets = [t.insert_order(*batches[0], stream=s_ord)]
        for i in range(len(batches)):
            if i + 1 < len(batches):
                tickets.append(t.insert_order(*batches[i + 1], stream=s_ord))
            t.insert_apply(tickets[i], stream=s_app)
            v = torch.empty_like(probe)
            f = torch.empty(probe.numel(), dtype=torch.uint8, device="cuda")
            t.search_batch(probe, v, f, stream=s_app)
            outs.append((v, f))
        t.synchronize()
    finally:
        proc.wait(timeout=60)
    assert proc.returncode == 0
    for (k, v), (gv, gf) in zip(batches, outs):
        orc.apply_batch(host(k), host(v))
        ov, of = orc.search_batch(probe_h)
        assert np.array_equal(host(gv), ov) and np.array_equal(gf.cpu().numpy(), of)
    assert t.last_error()["bits"] == 0
    compare_contents(t, orc)
    orc.close()
    t.close()
