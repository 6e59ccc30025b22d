"""shm_bulk_plan and shm_bulk_load at the C-ABI boundary, without a GPU: the
plan (host arithmetic) equals the numpy model's, both symbols are declared,
bound and exported unmangled, and rejected arguments return before the handle
or the GPU is used."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sherman_amd as shm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bulk_model as bm  # noqa: E402


def test_plan_equals_the_model_on_the_shapes():
    for n, lf, inf in bm.SHAPES:
        assert shm.bulk_plan(n, lf, inf) == bm.plan(n, lf, inf), (n, lf, inf)


def test_plan_equals_the_model_on_random_triples():
    rng = np.random.default_rng(20)
    done = 0
    while done < 200:
        n = int(rng.integers(0, (1 << 34) + 1)) >> int(rng.integers(0, 34))
        lf, inf = int(rng.integers(0, 54)), int(rng.integers(0, 61))
        if inf == 1:
            continue
        try:
            want = bm.plan(n, lf, inf)
        except ValueError:  # too tall: small fills under many keys
            with pytest.raises(shm.ShermanError) as e:
                shm.bulk_plan(n, lf, inf)
            assert e.value.rc == shm.SHM_EINVAL
        else:
            assert shm.bulk_plan(n, lf, inf) == want, (n, lf, inf)
        done += 1


def test_plan_rejects_bad_fills_and_tall_trees():
    p = shm.ShmBulkPlan()
    f = shm.lib().shm_bulk_plan
    for n, lf, inf in ((2188, 1, 2), (10, 54, 0), (10, 0, 1), (10, 0, 61), (10, 1 << 31, 0)):
        assert f(n, lf, inf, ctypes.byref(p)) == shm.SHM_EINVAL, (n, lf, inf)
        with pytest.raises(shm.ShermanError):
            shm.bulk_plan(n, lf, inf)
    assert f(10, 0, 0, None) == shm.SHM_EINVAL
    assert f(2187, 1, 2, ctypes.byref(p)) == shm.SHM_OK and p.root_level == 7
    assert list(p.level_pages) == [3 ** (7 - i) for i in range(8)] and p.pages == 3280
    assert f(0, 0, 0, ctypes.byref(p)) == shm.SHM_OK
    assert (p.pages, p.root_level, list(p.level_pages)) == (1, 0, [1] + [0] * 7)


def test_bulk_symbols_are_declared_bound_and_exported():
    sig = {n: (r, a) for n, r, a in shm._SIGNATURES}
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for name, nargs in (("shm_bulk_plan", 4), ("shm_bulk_load", 7)):
        assert name in shm.header_symbols()
        assert sig[name][0] is ctypes.c_int and len(sig[name][1]) == nargs
        assert re.search(r"\bT %s$" % name, out, re.M)  # unmangled => extern "C"
    assert ctypes.sizeof(shm.ShmBulkPlan) == 8 + 4 + 4 + 8 * 8
    assert hasattr(shm.Tree, "bulk_load") and callable(shm.bulk_plan)
    assert shm.lib().shm_abi_version() == shm.ABI_VERSION == 11  # additions only


def test_the_header_comment_states_the_contract():
    txt = open(shm.HEADER_PATH).read()
    at = txt.index("int shm_bulk_load(")
    comment = txt[txt.rindex("/*", 0, at):at]
    for word in ("strictly ascending", "Replace", "leaf_fill", "SHM_ENOMEM"):
        assert word in comment, word


def test_rejected_arguments_return_before_any_use_of_handle_or_gpu():
    """Null keys or vals with n > 0, fills out of range and a plan that is
    too tall are SHM_EINVAL on a null handle and on a handle that is no tree
    (a zeroed host buffer, which a call that went on would dereference)."""
    f = shm.lib().shm_bulk_load
    fake = ctypes.create_string_buffer(1 << 16)
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    for h in (None, ctypes.addressof(fake)):
        assert f(h, None, p, 1, 0, 0, None) == shm.SHM_EINVAL       # keys
        assert f(h, p, None, 1, 0, 0, None) == shm.SHM_EINVAL       # vals
        assert f(h, p, p, 1, 54, 0, None) == shm.SHM_EINVAL         # leaf_fill
        assert f(h, p, p, 1, 0, 1, None) == shm.SHM_EINVAL          # internal_fill
        assert f(h, p, p, 1, 0, 61, None) == shm.SHM_EINVAL
        assert f(h, None, None, 0, 54, 0, None) == shm.SHM_EINVAL   # also at n 0
        assert f(h, p, p, 2188, 1, 2, None) == shm.SHM_EINVAL       # too tall
    # a valid call on a null handle: still SHM_EINVAL, nothing touched
    assert f(None, p, p, 1, 0, 0, None) == shm.SHM_EINVAL
    assert f(None, None, None, 0, 0, 0, None) == shm.SHM_EINVAL
    assert all(x == 0 for x in buf)
    assert all(b == 0 for b in fake.raw)
