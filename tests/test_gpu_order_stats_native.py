"""Order statistics through the host C++ facade (sherman_amd/csrc/Tree.hpp
rank, count_range, select -> C-ABI -> HIP) against a std::map, as a C++
program (tests/native/order_test.cpp) run on the GPU."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_order_test():
    """The command line of tests/native/Makefile's recipe, for order_test;
    rebuilt when a source or the library is newer than the program."""
    exe = os.path.join(NATIVE, "_build", "order_test")
    deps = [os.path.join(NATIVE, "order_test.cpp"),
            os.path.join(ROOT, "sherman_amd", "csrc", "Tree.hpp"),
            os.path.join(ROOT, "include", "sherman_amd.h"),
            os.path.join(ROOT, "sherman_amd", "libsherman_amd.so")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    os.makedirs(os.path.join(NATIVE, "_build"), exist_ok=True)
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-o", "_build/order_test",
                           "order_test.cpp", "-L../../sherman_amd", "-lsherman_amd",
                           "-Wl,-rpath,$ORIGIN/../../../sherman_amd"], cwd=NATIVE)
    return exe


def test_native_order_test():
    exe = build_order_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "order_test ok" in r.stdout
