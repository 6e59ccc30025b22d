"""shm_scan_batch at the C-ABI boundary, without a GPU: the symbol is declared,
bound and exported unmangled, the ABI version did not move (the entry point
is an addition), rejected arguments return before the handle or the GPU is
used, and the numpy model the GPU tests compare against (tests/scan_model.py)
is itself checked on a hand-written key set."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

import sherman_amd as shm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scan_model import KEY_MAX, ScanModel  # noqa: E402

U64 = np.uint64


def test_scan_batch_is_declared_bound_and_exported():
    assert "shm_scan_batch" in shm.header_symbols()
    sig = {n: (r, a) for n, r, a in shm._SIGNATURES}
    assert "shm_scan_batch" in sig
    res, args = sig["shm_scan_batch"]
    assert res is ctypes.c_int and len(args) == 10
    assert args[3] is shm.u64 and args[4] is shm.u64  # n, limit
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT shm_scan_batch$", out, re.M)  # unmangled => extern "C"
    assert hasattr(shm.Tree, "scan_batch") and hasattr(shm.Tree, "lower_bound_batch")
    assert hasattr(shm, "PendingScan")


def test_abi_version_is_still_11():
    assert shm.lib().shm_abi_version() == shm.ABI_VERSION == 11
    txt = open(shm.HEADER_PATH).read()
    assert re.search(r"#define\s+SHM_ABI_VERSION\s+11\b", txt)


def test_rejected_arguments_return_before_any_use_of_handle_or_gpu():
    """limit == 0, limit >= 2^31 and null from / keys_out / vals_out /
    counts_out with n > 0 are SHM_EINVAL, and so is a null handle.  The
    argument checks come first: with a handle that is no tree (a zeroed host
    buffer, never dereferenced by a rejected call) they still return
    SHM_EINVAL, which a call that went on to the GPU could not."""
    f = shm.lib().shm_scan_batch
    fake = ctypes.create_string_buffer(1 << 16)
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    for h in (None, ctypes.addressof(fake)):
        assert f(h, p, None, 1, 0, p, p, p, None, None) == shm.SHM_EINVAL          # limit 0
        assert f(h, p, None, 1, 1 << 31, p, p, p, None, None) == shm.SHM_EINVAL    # limit 2^31
        assert f(h, p, None, 1, 1 << 40, p, p, p, None, None) == shm.SHM_EINVAL
        assert f(h, p, None, 0, 0, p, p, p, None, None) == shm.SHM_EINVAL          # also at n 0
        assert f(h, None, None, 1, 4, p, p, p, None, None) == shm.SHM_EINVAL       # from
        assert f(h, p, None, 1, 4, None, p, p, None, None) == shm.SHM_EINVAL       # keys_out
        assert f(h, p, None, 1, 4, p, None, p, None, None) == shm.SHM_EINVAL       # vals_out
        assert f(h, p, None, 1, 4, p, p, None, None, None) == shm.SHM_EINVAL       # counts_out
    # a valid call on a null handle: still SHM_EINVAL, nothing touched
    assert f(None, p, p, 1, (1 << 31) - 1, p, p, p, None, None) == shm.SHM_EINVAL
    assert f(None, None, None, 0, 1, None, None, None, None, None) == shm.SHM_EINVAL
    assert all(x == 0 for x in buf)


def test_scan_model_on_a_hand_written_key_set():
    """Eight keys on both sides of 2^63, given unsorted; every expected
    result below is written out by hand."""
    top = 1 << 63
    ks = np.array([top + 5, 10, 30, top, 20, KEY_MAX - 1, 40, top - 1], dtype=U64)
    vs = np.array([105, 1, 3, 100, 2, 999, 4, 99], dtype=U64)
    m = ScanModel(ks, vs)
    srt = [10, 20, 30, 40, top - 1, top, top + 5, KEY_MAX - 1]
    assert m.keys.tolist() == srt
    assert m.vals.tolist() == [1, 2, 3, 4, 99, 100, 105, 999]

    def one(lo, limit, hi=None):
        c, k, v, w = m.scan(np.array([lo], dtype=U64), limit,
                            None if hi is None else np.array([hi], dtype=U64))
        n = int(c[0])
        assert w[0].tolist() == [i < n for i in range(limit)]
        assert (k[0, n:] == 0).all() and (v[0, n:] == 0).all()
        return n, k[0, :n].tolist(), v[0, :n].tolist()

    assert one(0, 3) == (3, [10, 20, 30], [1, 2, 3])
    assert one(10, 1) == (1, [10], [1])                      # a stored key: itself
    assert one(11, 1) == (1, [20], [2])                      # a gap: the successor
    assert one(31, 4) == (4, [40, top - 1, top, top + 5], [4, 99, 100, 105])  # crosses 2^63
    assert one(top + 6, 5) == (1, [KEY_MAX - 1], [999])      # fewer than limit
    assert one(KEY_MAX - 1, 2) == (1, [KEY_MAX - 1], [999])
    assert one(KEY_MAX, 2) == (0, [], [])                    # no stored key equals it
    assert one(20, 9, hi=40) == (3, [20, 30, 40], [2, 3, 4])  # inclusive bound
    assert one(20, 2, hi=40) == (2, [20, 30], [2, 3])         # the limit cuts first
    assert one(21, 9, hi=29) == (0, [], [])                   # between two keys
    assert one(30, 9, hi=29) == (0, [], [])                   # from > to
    assert one(30, 9, hi=30) == (1, [30], [3])
    assert one(25, 9, hi=25) == (0, [], [])
    assert one(top - 1, 9, hi=top) == (2, [top - 1, top], [99, 100])
    # a batch, and the empty tree
    c, k, v, w = m.scan(np.array([0, 35, KEY_MAX], dtype=U64), 2)
    assert c.tolist() == [2, 2, 0] and k[1].tolist() == [40, top - 1]
    e = ScanModel(np.zeros(0, dtype=U64), np.zeros(0, dtype=U64))
    c, k, v, w = e.scan(np.array([0, 7], dtype=U64), 3)
    assert c.tolist() == [0, 0] and not w.any()
