"""The host arithmetic of the shard's exchanges (sherman_amd/csrc/shard_plan.h:
the get slot's capacity, the per-peer counts and offsets of the grouped
point-to-point rounds) for every rank of worlds 1 to 16 at once, from a C++
program of its own (tests/native/shard_plan_test.cpp).  Runs without a GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_shard_plan_test():
    """The command line of tests/native/Makefile's recipe; rebuilt when a
    source is newer than the program."""
    exe = os.path.join(NATIVE, "_build", "shard_plan_test")
    deps = [os.path.join(NATIVE, "shard_plan_test.cpp"),
            os.path.join(ROOT, "sherman_amd", "csrc", "shard_plan.h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    os.makedirs(os.path.join(NATIVE, "_build"), exist_ok=True)
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-Wall", "-o", "_build/shard_plan_test",
                           "shard_plan_test.cpp"], cwd=NATIVE)
    return exe


def test_native_shard_plan_test():
    exe = build_shard_plan_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shard_plan_test ok" in r.stdout


def test_plan_header_is_host_arithmetic_only():
    """shard_plan.h includes no HIP or RCCL header and nothing of the
    library's own, so the program above checks it as the library uses it."""
    src = open(os.path.join(ROOT, "sherman_amd", "csrc", "shard_plan.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs and all(i.startswith("<") for i in incs), incs
    assert not any("hip" in i or "rccl" in i for i in incs), incs
