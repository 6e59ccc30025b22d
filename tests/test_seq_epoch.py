"""The sequence hook's place in the C-ABI and the host arithmetic behind the
counters' periods; both run without a GPU.

* shm__seq_jump (tree_insert.cpp) is a test hook: the built library exports it,
  include/sherman_amd.h does not declare it;
* sherman_amd/csrc/seq_epoch.h (which clears a jump of a counter owes, the end
  of the chunk counter's epoch) against step-by-step models of the real
  streams, from a C++ program of its own (tests/native/seq_epoch_test.cpp).
"""
import os
import re
import subprocess

import sherman_amd as shm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_seq_jump_is_exported_and_not_in_the_public_header():
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT shm__seq_jump$", out, re.M), "the library lacks the hook"
    assert "shm__seq_jump" in {n for n, _, _ in shm._HOOKS}
    assert "shm__seq_jump" not in shm.header_symbols()
    assert "seq_jump" not in open(os.path.join(ROOT, "include", "sherman_amd.h")).read()


def build_seq_epoch_test():
    """The command line of tests/native/Makefile's recipe; rebuilt when a
    source is newer than the program."""
    exe = os.path.join(NATIVE, "_build", "seq_epoch_test")
    deps = [os.path.join(NATIVE, "seq_epoch_test.cpp"),
            os.path.join(ROOT, "sherman_amd", "csrc", "seq_epoch.h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    os.makedirs(os.path.join(NATIVE, "_build"), exist_ok=True)
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-Wall", "-o", "_build/seq_epoch_test",
                           "seq_epoch_test.cpp"], cwd=NATIVE)
    return exe


def test_native_seq_epoch_test():
    exe = build_seq_epoch_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "seq_epoch_test ok" in r.stdout
