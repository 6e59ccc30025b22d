"""shm_export and shm_compact at the C-ABI boundary, without a GPU: both
symbols are declared, bound and exported unmangled, the ABI number is
unchanged, the header states the contract, and rejected arguments return
before the handle or the GPU is used."""
import ctypes
import re
import subprocess

import sherman_amd as shm


def test_export_symbols_are_declared_bound_and_exported():
    sig = {n: (r, a) for n, r, a in shm._SIGNATURES}
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for name, nargs in (("shm_export", 8), ("shm_compact", 4)):
        assert name in shm.header_symbols()
        assert sig[name][0] is ctypes.c_int and len(sig[name][1]) == nargs
        assert re.search(r"\bT %s$" % name, out, re.M)  # unmangled => extern "C"
    for attr in ("export", "count", "compact"):
        assert callable(getattr(shm.Tree, attr))
    assert shm.lib().shm_abi_version() == shm.ABI_VERSION == 11  # additions only
    txt = open(shm.HEADER_PATH).read()
    assert re.search(r"#define SHM_ABI_VERSION 11\b", txt)


def comment_of(decl):
    txt = open(shm.HEADER_PATH).read()
    at = txt.index(decl)
    return txt[txt.rindex("/*", 0, at):at]


def test_the_header_comments_state_the_contract():
    c = comment_of("int shm_export(")
    for word in ("ascending", "shm_scan_batch", "kValueNull", "lo > hi", "NULL", "SHM_ENOSPC",
                 "nothing is written", "no word past", "synchronising", "Read-only", "SHM_EINVAL",
                 "SHM_ENOMEM", "SHM_EIO", "torn", "VALID"):
        assert word in c, word
    c = comment_of("int shm_compact(")
    for word in ("shm_bulk_load", "shm_bulk_plan", "36 / 40", "pages_used == plan.pages",
                 "versions restart at 1", "directory", "byte for byte", "SHM_EINVAL", "SHM_ENOMEM",
                 "shm_insert_order", "Exclusive"):
        assert word in c, word


def test_rejected_arguments_return_before_any_use_of_handle_or_gpu():
    """A null handle and a null n_out are SHM_EINVAL for shm_export, fills out
    of range for shm_compact, on a null handle and on a handle that is no tree
    (a zeroed host buffer, which a call that went on would dereference and
    lock).  Whether a plan is too tall depends on the number of valid pairs,
    which only the tree knows: that rejection is tested on the GPU."""
    ex, co = shm.lib().shm_export, shm.lib().shm_compact
    fake = ctypes.create_string_buffer(1 << 16)
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    n = ctypes.c_uint64(77)
    kmax = (1 << 64) - 1
    for h in (None, ctypes.addressof(fake)):
        assert ex(h, 0, kmax, p, p, 8, None, None) == shm.SHM_EINVAL   # n_out
        assert ex(h, 0, kmax, None, None, 0, None, None) == shm.SHM_EINVAL
        assert co(h, 54, 0, None) == shm.SHM_EINVAL                    # leaf_fill
        assert co(h, 0, 1, None) == shm.SHM_EINVAL                     # internal_fill
        assert co(h, 0, 61, None) == shm.SHM_EINVAL
        assert co(h, 1 << 31, 0, None) == shm.SHM_EINVAL
    assert ex(None, 0, kmax, p, p, 8, ctypes.byref(n), None) == shm.SHM_EINVAL
    assert ex(None, 5, 1, None, None, 0, ctypes.byref(n), None) == shm.SHM_EINVAL
    assert co(None, 0, 0, None) == shm.SHM_EINVAL
    assert co(None, 53, 60, None) == shm.SHM_EINVAL
    assert n.value == 77
    assert all(x == 0 for x in buf)
    assert all(b == 0 for b in fake.raw)
