"""The routed get's slot placement alone, with and without splitters, at the
C4 shard size: 2^20 hashed queries into P runs (shm__route_slots_ex: equal
slices; shm__route_slots_bounds: splitters, the owner search from the kernel
arguments and from LDS), and the stable bucketing of the same keys
(shm_route_bucket / shm__route_bucket_mode).  The splitters are the equal
slices' own boundaries, so every form does the same work apart from the owner
search.  Each figure is the median of `reps` timings of `steps` launches
between two HIP events, with the lowest and highest beside it: the spread a
comparison has to clear.  No tree is walked and nothing is exchanged.

An older build of the library under SHM_LIB_PATH (no splitter hooks) gives
the equal-slice figures alone: the parent's side of profiles/route_bounds.json.
usage: python tools/route_bounds.py [steps] [reps] [P ...]"""
import ctypes
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sherman_amd as shm

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
worlds = [int(x) for x in sys.argv[3:]] or [8, 16, 64]
torch.cuda.set_device(0)
batch = 1 << 20
vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
L = shm.lib()
L.shm__route_slots_ex.restype = ci
L.shm__route_slots_ex.argtypes = [vp, vp, u64, u32, u64, vp, vp, vp, vp, vp, ci, vp]
bounds = hasattr(L, "shm__route_slots_bounds")
if bounds:
    L.shm__route_slots_bounds.restype = ci
    L.shm__route_slots_bounds.argtypes = [vp, vp, u64, u32, u64, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.shm__route_bucket_mode.restype = ci
    L.shm__route_bucket_mode.argtypes = [vp, vp, u64, u32, vp, ci, vp, vp, vp, vp]

t = shm.Tree(arena_bytes=16 << 20, max_batch=batch)
ids = torch.randint(1, 1 << 27, (4, batch), device="cuda")
qs = []
for i in range(4):
    q = torch.empty(batch, dtype=torch.int64, device="cuda")
    t.hash_keys(ids[i], q)
    qs.append(q)
sp = torch.cuda.current_stream().cuda_stream


def timed(fn):
    for i in range(10):
        fn(i)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(steps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return {"us": round(statistics.median(out), 2), "min": round(min(out), 2),
            "max": round(max(out), 2)}


res = {"batch": batch, "steps": steps, "reps": reps, "lib": os.path.basename(os.path.dirname(
    os.path.abspath(shm.LIB_PATH))), "splitter_hooks": bounds, "worlds": {}}
for P in worlds:
    cap = batch // P + 6 * int(math.sqrt(batch // P)) + 256  # shard.cpp get_slot_cap
    cursor = torch.zeros(P + 1, dtype=torch.int32, device="cuda")
    slots = torch.empty(P * cap, dtype=torch.int64, device="cuda")
    spos = torch.empty(batch, dtype=torch.int32, device="cuda")
    ovk = torch.zeros(batch, dtype=torch.int64, device="cuda")
    ovi = torch.zeros(batch, dtype=torch.int32, device="cuda")
    ko = torch.empty(batch, dtype=torch.int64, device="cuda")
    perm = torch.empty(batch, dtype=torch.int32, device="cuda")
    cnt = torch.empty(P, dtype=torch.int64, device="cuda")
    eq = [((p << 64) + P - 1) // P for p in range(1, P)]
    arr = (u64 * max(len(eq), 1))(*eq)

    def slots_equal(i):
        assert L.shm__route_slots_ex(t.h, qs[i % 4].data_ptr(), batch, P, cap, cursor.data_ptr(),
                                     slots.data_ptr(), spos.data_ptr(), ovk.data_ptr(),
                                     ovi.data_ptr(), 1 if i == 0 else 0, sp) == 0

    def slots_split(mode):
        def fn(i):
            assert L.shm__route_slots_bounds(t.h, qs[i % 4].data_ptr(), batch, P, cap,
                                             cursor.data_ptr(), slots.data_ptr(), spos.data_ptr(),
                                             ovk.data_ptr(), ovi.data_ptr(), 1 if i == 0 else 0,
                                             arr, mode, sp) == 0
        return fn

    def bucket_equal(i):
        t.route_bucket(qs[i % 4], P, ko, perm, cnt)

    def bucket_split(mode):
        def fn(i):
            assert L.shm__route_bucket_mode(t.h, qs[i % 4].data_ptr(), batch, P, arr, mode,
                                            cnt.data_ptr(), ko.data_ptr(), perm.data_ptr(), sp) == 0
        return fn

    w = {"cap": cap, "slots_equal": timed(slots_equal), "bucket_equal": timed(bucket_equal)}
    base = spos.clone()
    if bounds:
        if P <= 16:
            w["slots_split_args"] = timed(slots_split(1))
            w["bucket_split_args"] = timed(bucket_split(1))
        w["slots_split_lds"] = timed(slots_split(2))
        w["bucket_split_lds"] = timed(bucket_split(2))
        w["slots_equal_again"] = timed(slots_equal)
        # the same owners either way: the same slot run for every key
        slots_equal(1)
        a = spos.clone() // cap
        slots_split(2)(1)
        torch.cuda.synchronize()
        assert torch.equal(a, spos // cap), "splitter owners differ from the equal slices'"
    assert int(cursor[P].item()) == 0, "overflow at this capacity"
    res["worlds"][str(P)] = w
t.synchronize()
print(json.dumps(res))
