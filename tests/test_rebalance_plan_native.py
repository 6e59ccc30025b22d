"""shm_rebalance_plan from a C++ program of its own
(tests/native/rebalance_plan_test.cpp): host arithmetic, so it runs without a
GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_plan_test():
    """The command line of tests/native/Makefile's recipe, for
    rebalance_plan_test; rebuilt when a source or the library is newer than
    the program."""
    exe = os.path.join(NATIVE, "_build", "rebalance_plan_test")
    deps = [os.path.join(NATIVE, "rebalance_plan_test.cpp"),
            os.path.join(ROOT, "include", "sherman_amd.h"),
            os.path.join(ROOT, "sherman_amd", "libsherman_amd.so")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    os.makedirs(os.path.join(NATIVE, "_build"), exist_ok=True)
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-o", "_build/rebalance_plan_test",
                           "rebalance_plan_test.cpp", "-L../../sherman_amd", "-lsherman_amd",
                           "-Wl,-rpath,$ORIGIN/../../../sherman_amd"], cwd=NATIVE)
    return exe


def test_native_rebalance_plan_test():
    exe = build_plan_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rebalance_plan_test ok" in r.stdout
