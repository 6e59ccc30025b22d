"""shm_rank_batch, shm_count_batch, shm_select_batch and shm_order_stats at the
C-ABI boundary, without a GPU: the symbols are declared, bound and exported
unmangled, the ABI number is unchanged, the header states the contract, and
rejected arguments return before the handle or the GPU is used."""
import ctypes
import re
import subprocess

import sherman_amd as shm

CALLS = (("shm_rank_batch", 6), ("shm_count_batch", 7), ("shm_select_batch", 8),
         ("shm_order_stats", 2))


def test_order_symbols_are_declared_bound_and_exported():
    sig = {n: (r, a) for n, r, a in shm._SIGNATURES}
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for name, nargs in CALLS:
        assert name in shm.header_symbols()
        assert sig[name][0] is ctypes.c_int and len(sig[name][1]) == nargs
        assert re.search(r"\bT %s$" % name, out, re.M)  # unmangled => extern "C"
    for attr in ("rank_batch", "count_batch", "select_batch", "order_stats", "quantile_keys"):
        assert callable(getattr(shm.Tree, attr))
    assert shm.lib().shm_abi_version() == shm.ABI_VERSION == 11  # additions only
    txt = open(shm.HEADER_PATH).read()
    assert re.search(r"#define SHM_ABI_VERSION 11\b", txt)
    assert ctypes.sizeof(shm.ShmOrderStats) == 40


def test_the_host_side_of_the_index_is_not_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"shm4host\w*order_", out)


def test_the_header_comment_states_the_contract():
    txt = open(shm.HEADER_PATH).read()
    at = txt.index("int shm_rank_batch(")
    c = txt[txt.rindex("/* Order statistics", 0, at):at]
    for word in ("shm_export(0, keys[i] - 1)", "shm_export(0, kKeyMax)", "kKeyMax", "torn",
                 "src/Tree.cpp:461-540", "DEVICE", "n == 0", "not all three", "shm_insert_order",
                 "status_dev[1]", "exclusive", "synchronising", "without a", "SHM_EINVAL",
                 "SHM_ENOMEM", "SHM_EIO", "shm_range_query", "shm_load_image", "read-only"):
        assert word in c, word


def test_rejected_arguments_return_before_any_use_of_handle_or_gpu():
    """A null handle and a null required array with n > 0 are SHM_EINVAL, on a
    null handle and on a handle that is no tree (a zeroed host buffer, which a
    call that went on would dereference and lock).  The outstanding-ticket
    rejection needs a tree: it is tested on the GPU."""
    L = shm.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    for h in (None, ctypes.addressof(fake)):
        assert L.shm_rank_batch(h, None, 4, p, None, None) == shm.SHM_EINVAL
        assert L.shm_rank_batch(h, p, 4, None, None, None) == shm.SHM_EINVAL
        assert L.shm_count_batch(h, None, p, 4, p, None, None) == shm.SHM_EINVAL
        assert L.shm_count_batch(h, p, None, 4, p, None, None) == shm.SHM_EINVAL
        assert L.shm_count_batch(h, p, p, 4, None, None, None) == shm.SHM_EINVAL
        assert L.shm_select_batch(h, None, 4, p, p, p, None, None) == shm.SHM_EINVAL
        assert L.shm_select_batch(h, p, 4, None, None, None, None, None) == shm.SHM_EINVAL
    st = shm.ShmOrderStats()
    assert L.shm_rank_batch(None, p, 4, p, None, None) == shm.SHM_EINVAL
    assert L.shm_rank_batch(None, p, 0, p, None, None) == shm.SHM_EINVAL
    assert L.shm_count_batch(None, p, p, 4, p, None, None) == shm.SHM_EINVAL
    assert L.shm_select_batch(None, p, 4, p, None, None, None, None) == shm.SHM_EINVAL
    assert L.shm_order_stats(None, ctypes.byref(st)) == shm.SHM_EINVAL
    assert L.shm_order_stats(ctypes.addressof(fake), None) == shm.SHM_EINVAL
    assert all(x == 0 for x in buf)
    assert all(b == 0 for b in fake.raw)
