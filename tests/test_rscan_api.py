"""shm_rscan_batch at the C-ABI boundary, without a GPU: the symbol is
declared, bound and exported unmangled, rejected arguments return before the
handle or the GPU is used, and the numpy model the GPU tests compare against
(tests/rscan_model.py) is itself checked on a hand-written key set."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

import sherman_amd as shm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rscan_model import KEY_MAX, RScanModel  # noqa: E402

U64 = np.uint64


def test_rscan_batch_is_declared_bound_and_exported():
    assert "shm_rscan_batch" in shm.header_symbols()
    sig = {n: (r, a) for n, r, a in shm._SIGNATURES}
    assert "shm_rscan_batch" in sig
    res, args = sig["shm_rscan_batch"]
    assert res is ctypes.c_int and len(args) == 10
    assert args[3] is shm.u64 and args[4] is shm.u64  # n, limit
    assert sig["shm_rscan_batch"] == sig["shm_scan_batch"]
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT shm_rscan_batch$", out, re.M)  # unmangled => extern "C"
    assert hasattr(shm.Tree, "rscan_batch") and hasattr(shm.Tree, "floor_batch")
    assert shm.lib().shm_abi_version() == shm.ABI_VERSION == 11  # an addition


def test_the_header_comment_states_the_contract():
    txt = open(shm.HEADER_PATH).read()
    at = txt.index("int shm_rscan_batch(")
    comment = txt[txt.rindex("/*", 0, at):at]
    for word in ("DESCENDING", "kKeyMax", "stop of 0", "last key - 1"):
        assert word in comment, word


def test_rejected_arguments_return_before_any_use_of_handle_or_gpu():
    """The cases of test_scan_api.py: limit == 0, limit >= 2^31 and null from
    / keys_out / vals_out / counts_out with n > 0 are SHM_EINVAL, and so is a
    null handle.  With a handle that is no tree (a zeroed host buffer, never
    dereferenced by a rejected call) they still return SHM_EINVAL, which a
    call that went on to the GPU could not."""
    f = shm.lib().shm_rscan_batch
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
    assert all(b == 0 for b in fake.raw)


def test_rscan_model_on_a_hand_written_key_set():
    """Eight keys on both sides of 2^63, given unsorted; every expected
    result below is written out by hand."""
    top = 1 << 63
    ks = np.array([top + 5, 10, 30, top, 20, KEY_MAX - 1, 40, top - 1], dtype=U64)
    vs = np.array([105, 1, 3, 100, 2, 999, 4, 99], dtype=U64)
    m = RScanModel(ks, vs)
    assert m.keys.tolist() == [10, 20, 30, 40, top - 1, top, top + 5, KEY_MAX - 1]
    assert m.vals.tolist() == [1, 2, 3, 4, 99, 100, 105, 999]

    def one(start, limit, stop=None):
        c, k, v, w = m.scan(np.array([start], dtype=U64), limit,
                            None if stop is None else np.array([stop], dtype=U64))
        n = int(c[0])
        assert w[0].tolist() == [i < n for i in range(limit)]
        assert (k[0, n:] == 0).all() and (v[0, n:] == 0).all()
        return n, k[0, :n].tolist(), v[0, :n].tolist()

    assert one(30, 1) == (1, [30], [3])                      # a stored key: itself
    assert one(30, 5) == (3, [30, 20, 10], [3, 2, 1])        # fewer than limit
    assert one(29, 1) == (1, [20], [2])                      # a gap: the predecessor
    assert one(39, 2) == (2, [30, 20], [3, 2])
    assert one(9, 3) == (0, [], [])                          # below the minimum
    assert one(0, 3) == (0, [], [])
    assert one(KEY_MAX, 2) == (2, [KEY_MAX - 1, top + 5], [999, 105])  # from the largest key
    assert one(KEY_MAX - 1, 1) == (1, [KEY_MAX - 1], [999])
    assert one(KEY_MAX - 2, 1) == (1, [top + 5], [105])
    assert one(top + 4, 4) == (4, [top, top - 1, 40, 30], [100, 99, 4, 3])  # crosses 2^63 downward
    assert one(40, 9, stop=20) == (3, [40, 30, 20], [4, 3, 2])  # inclusive stop
    assert one(40, 2, stop=20) == (2, [40, 30], [4, 3])         # the limit cuts first
    assert one(29, 9, stop=21) == (0, [], [])                   # between two keys
    assert one(29, 9, stop=30) == (0, [], [])                   # stop > start
    assert one(10, 9, stop=KEY_MAX) == (0, [], [])
    assert one(30, 9, stop=30) == (1, [30], [3])
    assert one(25, 9, stop=25) == (0, [], [])
    assert one(top, 9, stop=top - 1) == (2, [top, top - 1], [100, 99])
    assert one(KEY_MAX, 9, stop=top + 1) == (2, [KEY_MAX - 1, top + 5], [999, 105])
    # a batch, and the empty tree
    c, k, v, w = m.scan(np.array([0, 35, KEY_MAX], dtype=U64), 2)
    assert c.tolist() == [0, 2, 2] and k[1].tolist() == [30, 20]
    assert k[2].tolist() == [KEY_MAX - 1, top + 5]
    e = RScanModel(np.zeros(0, dtype=U64), np.zeros(0, dtype=U64))
    c, k, v, w = e.scan(np.array([0, 7, KEY_MAX], dtype=U64), 3)
    assert c.tolist() == [0, 0, 0] and not w.any()
