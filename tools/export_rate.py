#!/usr/bin/env python3
"""Rate of the sorted export (Tree.export) and of the compaction built on it,
beside the only other way to the same pairs: one scan_batch from key 0.

Trees timed: 2^k hashed keys (gen_keys 1..N, values 2 * id) for k in
--log2-keys (24, 26), made by bulk_load at each of --fills (36/40, 53/60),
and the 2^--insert-log2 (24) tree built by insert_batch chunks of 2^20 in
generation order, whose pages lie in arbitrary order.

Per tree: device events around the whole shm_export call into buffers that
fit (expansion, leaf count pass, the host's read of the total, leaf write
pass), --runs runs after a warm-up, the best and the spread; the count-only
call the same way (its difference to the full call is the write pass);
compact() beside export + bulk_load of the exported pairs.  Reported: keys/s,
bytes per key -- written: 16 B per pair; read: every leaf in range twice, at
most 1024 B each time (768 B where the leaf's occupancy bound ends before
slot 40) -- and the sum of both per second as a share of the device fill rate
calibrated in the same process (a fill of --cal-bytes, best of 5).

Yardstick: scan_batch(from = 0, limit = n) on trees of 2^k keys for k in
--scan-log2 (20, 24), timed the same way, and the ratio.

--trace K: nothing of the above; 2^K keys loaded at the first of --fills and
exported --runs + 1 times, for a run of its own under the profiler (rocprofv3
--kernel-trace --stats -- python tools/export_rate.py --trace 26): the
k_export_* rows of its kernel statistics are the per-kernel split.

There is no fallback: without a GPU the tool fails.  Writes --out
(profiles/export_rate.json) and prints the table.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAGE = 1024


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log2-keys", type=int, nargs="+", default=[24, 26])
    ap.add_argument("--insert-log2", type=int, default=24)
    ap.add_argument("--scan-log2", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--fills", type=str, nargs="+", default=["36/40", "53/60"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cal-bytes", type=int, default=4 << 30)
    ap.add_argument("--trace", type=int, default=None,
                    help="only export a loaded tree of 2^K keys (a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_rate.json"))
    a = ap.parse_args(argv)
    a.fills = [tuple(int(x) for x in f.split("/")) for f in a.fills]
    if a.runs < 1 or min(a.log2_keys + a.scan_log2 + [a.insert_log2]) < 10:
        ap.error("runs must be positive and sizes at least 2^10")
    return a


def timed(torch, fn):
    """device ms between events around fn"""
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate_write(torch, nbytes):
    buf = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    buf.zero_()
    best = min(timed(torch, buf.zero_) for _ in range(5))
    del buf
    return nbytes / (best * 1e-3)


def hashed(torch, t, N):
    gen = torch.empty(N, dtype=torch.int64, device="cuda")
    for first in range(0, N, 1 << 22):
        m = min(1 << 22, N - first)
        t.gen_keys(first + 1, m, gen[first:first + m])
    ids2 = torch.arange(1, N + 1, dtype=torch.int64, device="cuda") * 2
    return gen, ids2


def usorted(torch, gen, ids2):
    top = -(1 << 63)  # unsigned order: flip the top bit around a signed sort
    sk, order = torch.sort(gen ^ top)
    sk ^= top
    return sk, ids2[order]


def measure(torch, shm, t, N, sk, sv, runs, cal, what, lf, inf):
    ko = torch.empty(N, dtype=torch.int64, device="cuda")
    vo = torch.empty(N, dtype=torch.int64, device="cuda")
    full = [timed(torch, lambda: t.export(keys=ko, vals=vo)) for _ in range(runs + 1)][1:]
    assert bool((ko == sk).all()) and bool((vo == sv).all()), what
    count = [timed(torch, lambda: t.count()) for _ in range(runs + 1)][1:]
    st = t.stats()
    leaves = t.check()["leaves"] if N <= (1 << 24) else shm.bulk_plan(N, lf, inf)["level_pages"][0]
    best = min(full)
    rd, wr = 2 * PAGE * leaves, 16 * N
    row = {"tree": what, "log2_keys": N.bit_length() - 1, "pages": st["pages_used"],
           "leaves": leaves, "root_level": st["root_level"],
           "export_ms": [round(m, 3) for m in full], "count_ms": [round(m, 3) for m in count],
           "keys_per_s": N / (best * 1e-3), "spread": (max(full) - best) / best,
           "written_bytes_per_key": wr / N, "read_bytes_per_key_at_most": rd / N,
           "bytes_per_s": (rd + wr) / (best * 1e-3),
           "of_calibrated_fill": (rd + wr) / (best * 1e-3) / cal,
           "write_pass_ms": round(best - min(count), 3)}
    print(f"{what}: export {best:.3f} ms, count {min(count):.3f} ms", flush=True)
    return row, ko, vo


def main(argv=None):
    args = parse(argv)
    import torch

    import sherman_amd as shm

    if not torch.cuda.is_available():
        raise SystemExit("export_rate needs a GPU (no fallback)")
    if args.trace is not None:
        N = 1 << args.trace
        t = shm.Tree(arena_bytes=max(1 << 30, N * 64), max_batch=1 << 20)
        sk, sv = usorted(torch, *hashed(torch, t, N))
        t.bulk_load(sk, sv, *args.fills[0])
        ko, vo = torch.empty_like(sk), torch.empty_like(sv)
        for _ in range(args.runs + 1):
            t.export(keys=ko, vals=vo)
        assert bool((ko == sk).all()) and bool((vo == sv).all())
        print(f"exported 2^{args.trace} keys {args.runs + 1} times")
        t.close()
        return
    cal = calibrate_write(torch, args.cal_bytes)
    print(f"calibrated fill rate {cal / 1e9:.0f} GB/s", flush=True)
    rows, scans = [], []
    for lg in args.log2_keys:
        N = 1 << lg
        t = shm.Tree(arena_bytes=max(1 << 30, N * 64), max_batch=1 << 20)
        gen, ids2 = hashed(torch, t, N)
        sk, sv = usorted(torch, gen, ids2)
        del gen, ids2
        for lf, inf in args.fills:
            t.bulk_load(sk, sv, lf, inf)
            row, ko, vo = measure(torch, shm, t, N, sk, sv, args.runs, cal,
                                  f"2^{lg} bulk {lf}/{inf}", lf, inf)
            # compaction beside its two halves
            row["compact_ms"] = round(timed(torch, lambda: t.compact(lf, inf)), 3)
            row["export_plus_load_ms"] = round(
                timed(torch, lambda: t.bulk_load(*t.export(keys=ko, vals=vo), lf, inf)), 3)
            rows.append(row)
            if lg in args.scan_log2:
                scans.append(scan_row(torch, t, N, sk, sv, min(row["export_ms"])))
            del ko, vo
        t.close()
        del sk, sv
    for lg in sorted(set(args.scan_log2) - set(args.log2_keys)):
        N = 1 << lg
        t = shm.Tree(arena_bytes=max(1 << 30, N * 64), max_batch=1 << 20)
        sk, sv = usorted(torch, *hashed(torch, t, N))
        t.bulk_load(sk, sv)
        ko, vo = torch.empty_like(sk), torch.empty_like(sv)
        ex = min(timed(torch, lambda: t.export(keys=ko, vals=vo)) for _ in range(args.runs + 1))
        scans.append(scan_row(torch, t, N, sk, sv, ex))
        t.close()
    N = 1 << args.insert_log2
    t = shm.Tree(arena_bytes=max(1 << 30, N * 64), max_batch=1 << 20)
    gen, ids2 = hashed(torch, t, N)
    for c in range(0, N, 1 << 20):
        t.insert_batch(gen[c:c + (1 << 20)], ids2[c:c + (1 << 20)])
    sk, sv = usorted(torch, gen, ids2)
    del gen, ids2
    row, ko, vo = measure(torch, shm, t, N, sk, sv, args.runs, cal,
                          f"2^{args.insert_log2} built by inserts", 0, 0)
    before = t.stats()["pages_used"]
    row["compact_ms"] = round(timed(torch, lambda: t.compact(53, 60)), 3)
    row["pages_after_compact_53_60"] = t.stats()["pages_used"]
    assert row["pages_after_compact_53_60"] < before
    rows.append(row)
    t.close()
    res = {"tool": "tools/export_rate.py", "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "calibrated_fill_GB_per_s": cal / 1e9,
           "calibration": "device fill of %d bytes, best of 5, same process" % args.cal_bytes,
           "bytes_are": "algorithmic: 16 B per pair written; every leaf read twice, counted "
                        "as 1024 B each time (an upper bound: 768 B where the occupancy "
                        "bound ends before slot 40)",
           "times_are": "device events around the whole call; shm_export waits for the "
                        "count before the write pass and for the outputs before it returns",
           "rows": rows, "scan_yardstick": scans}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"{'tree':<26} {'ms':>9} {'count ms':>9} {'Gkeys/s':>8} {'B/key rd':>8} {'GB/s':>7} "
          f"{'of fill':>7} {'spread':>7} {'compact':>9} {'exp+load':>9}")
    for r in rows:
        print(f"{r['tree']:<26} {min(r['export_ms']):>9.3f} {min(r['count_ms']):>9.3f} "
              f"{r['keys_per_s'] / 1e9:>8.2f} {r['read_bytes_per_key_at_most']:>8.1f} "
              f"{r['bytes_per_s'] / 1e9:>7.0f} {r['of_calibrated_fill']:>7.2f} {r['spread']:>7.3f} "
              f"{r['compact_ms']:>9.3f} {r.get('export_plus_load_ms', float('nan')):>9.3f}")
    for s in scans:
        print(f"2^{s['log2_keys']} one scan_batch from 0: {s['scan_ms']:.1f} ms, export "
              f"{s['export_ms']:.3f} ms: {s['scan_over_export']:.0f} x")


def scan_row(torch, t, N, sk, sv, export_ms):
    """the parent's only way to the same pairs: one scan from key 0"""
    lo = torch.zeros(1, dtype=torch.int64, device="cuda")
    ko = torch.empty(N, dtype=torch.int64, device="cuda")
    vo = torch.empty(N, dtype=torch.int64, device="cuda")

    def scan():
        t.scan_batch(lo, N, keys=ko, vals=vo).check()

    ms = min(timed(torch, scan) for _ in range(2))
    assert bool((ko == sk).all()) and bool((vo == sv).all())
    print(f"2^{N.bit_length() - 1} scan_batch from 0: {ms:.1f} ms", flush=True)
    return {"log2_keys": N.bit_length() - 1, "scan_ms": round(ms, 3),
            "export_ms": round(export_ms, 3), "scan_over_export": ms / export_ms}


if __name__ == "__main__":
    main()
