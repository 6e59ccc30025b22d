"""The shared page readers (sherman_amd/csrc/page_fields.h: the header, the
u64 that starts at byte 1 of a dword, an internal record's key and pointer)
against byte-wise reads at layout.h's offsets, from a C++ program of its own
(tests/native/page_fields_test.cpp).  Runs without a GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_page_fields_test():
    """The command line of tests/native/Makefile's recipe; rebuilt when a
    source is newer than the program."""
    exe = os.path.join(NATIVE, "_build", "page_fields_test")
    deps = [os.path.join(NATIVE, "page_fields_test.cpp"),
            os.path.join(ROOT, "sherman_amd", "csrc", "page_fields.h"),
            os.path.join(ROOT, "sherman_amd", "csrc", "layout.h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    os.makedirs(os.path.join(NATIVE, "_build"), exist_ok=True)
    subprocess.check_call([HIPCC, "-x", "c++", "-O2", "-std=c++17", "-Wall", "-o", "_build/page_fields_test",
                           "page_fields_test.cpp"], cwd=NATIVE)
    return exe


def test_native_page_fields_test():
    exe = build_page_fields_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "page_fields_test ok" in r.stdout


def test_page_fields_header_is_plain_cpp():
    """page_fields.h includes layout.h and nothing else (no HIP header), so
    the program above checks the readers as the kernels and the host use
    them."""
    src = open(os.path.join(ROOT, "sherman_amd", "csrc", "page_fields.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ['"layout.h"'], incs
