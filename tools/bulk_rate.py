#!/usr/bin/env python3
"""Rate of the bulk load (Tree.bulk_load) beside the build of the same key
set by inserts, as bench.py's build_shard does it.

Workload: 2^k hashed keys (gen_keys 1..N, values 2 * id) for k in --log2-keys
(24, 26), sorted on the device (unsigned) before the timed part.  Per size
and per (leaf_fill, internal_fill) in --fills (36/40, 53/60):

  bulk         bulk_load of the sorted pairs: device events around the call
               (check pass, leaves, levels, superblock), --runs runs on one
               tree, the best run and the spread
  insert       the same pairs in generation order through insert_batch in
               chunks of 2^20 on a fresh tree, device events around the whole
               build, --insert-runs runs; in the same process on the same GPU

Reported per case: keys/s, the algorithmic bytes per key -- written: (1024 B
page + 64 B summary line) per leaf + 1024 B per internal page, over N; read:
16 B per pair by the check and 16 B by the leaves -- the written bytes per
second as a fraction of the streaming write rate calibrated in the same
process (a device memset of --cal-bytes, best of 5), and the ratio to the
insert build.

There is no fallback: without a GPU the tool fails.  Writes --out
(profiles/bulk_rate.json) and prints the table.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAGE, SUM_LINE = 1024, 64


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log2-keys", type=int, nargs="+", default=[24, 26])
    ap.add_argument("--fills", type=str, nargs="+", default=["36/40", "53/60"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--insert-runs", type=int, default=2)
    ap.add_argument("--cal-bytes", type=int, default=4 << 30)
    ap.add_argument("--check-max", type=int, default=1 << 24,
                    help="largest key count whose trees get the structural check (a host copy)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bulk_rate.json"))
    a = ap.parse_args(argv)
    a.fills = [tuple(int(x) for x in f.split("/")) for f in a.fills]
    if a.runs < 1 or a.insert_runs < 1 or min(a.log2_keys) < 10:
        ap.error("runs must be positive and sizes at least 2^10")
    return a


def load_bytes(plan, n):
    """(written, read) algorithmic bytes of one load"""
    leaves = plan["level_pages"][0]
    return plan["pages"] * PAGE + leaves * SUM_LINE, 32 * n


def timed(torch, fn):
    """(device ms between events around fn, host ms until the device is done)"""
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def calibrate_write(torch, nbytes):
    """streaming write rate: a device fill of nbytes, best of 5 (bytes/s)"""
    buf = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    buf.zero_()
    best = min(timed(torch, buf.zero_)[0] for _ in range(5))
    del buf
    return nbytes / (best * 1e-3)


def main(argv=None):
    args = parse(argv)
    import torch

    import sherman_amd as shm

    if not torch.cuda.is_available():
        raise SystemExit("bulk_rate needs a GPU (no fallback)")
    dev = "cuda"
    cal = calibrate_write(torch, args.cal_bytes)
    print(f"calibrated write rate {cal / 1e9:.0f} GB/s", flush=True)
    top = -(1 << 63)
    rows = []
    for lg in args.log2_keys:
        N = 1 << lg
        arena = max(1 << 30, N * 64)
        t = shm.Tree(arena_bytes=arena, max_batch=1 << 20)
        gen = torch.empty(N, dtype=torch.int64, device=dev)
        for first in range(0, N, 1 << 22):
            m = min(1 << 22, N - first)
            t.gen_keys(first + 1, m, gen[first:first + m])
        ids2 = torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 2
        # unsigned order: flip the top bit around a signed sort
        sk, order = torch.sort(gen ^ top)
        sk ^= top
        sv = ids2[order]
        del order
        torch.cuda.synchronize()
        # the insert build, as build_shard: generation order, chunks of 2^20
        ins_ms = []
        for _ in range(args.insert_runs):
            ti = shm.Tree(arena_bytes=arena, max_batch=1 << 20)

            def build():
                for c in range(0, N, 1 << 20):
                    ti.insert_batch(gen[c:c + (1 << 20)], ids2[c:c + (1 << 20)])

            ins_ms.append(timed(torch, build))
            ins_pages = ti.stats()["pages_used"]
            if N <= args.check_max:  # the structural check copies the arena to the host
                assert ti.check()["keys"] == N
            ti.close()
            print(f"2^{lg} insert build: {ins_ms[-1][0]:.1f} ms, {ins_pages} pages", flush=True)
        ins_best = min(m for m, _ in ins_ms)
        for lf, inf in args.fills:
            plan = shm.bulk_plan(N, lf, inf)
            ms = [timed(torch, lambda: t.bulk_load(sk, sv, lf, inf)) for _ in range(args.runs + 1)][1:]
            assert t.stats()["pages_used"] == plan["pages"]
            if N <= args.check_max:
                st = t.check()
                assert st == {"leaves": plan["level_pages"][0],
                              "internal": plan["pages"] - plan["level_pages"][0], "keys": N}, st
            out = torch.empty(1 << 20, dtype=torch.int64, device=dev)
            t.search_batch(gen[:1 << 20], out)
            t.synchronize()
            assert bool((out == ids2[:1 << 20]).all())
            best = min(m for m, _ in ms)
            wr, rd = load_bytes(plan, N)
            rows.append({
                "log2_keys": lg, "leaf_fill": lf, "internal_fill": inf, "pages": plan["pages"],
                "root_level": plan["root_level"],
                "bulk_ms": [round(m, 3) for m, _ in ms], "bulk_host_ms": [round(h, 3) for _, h in ms],
                "keys_per_s": N / (best * 1e-3),
                "spread": (max(m for m, _ in ms) - best) / best,
                "written_bytes_per_key": wr / N, "read_bytes_per_key": rd / N,
                "written_bytes_per_s": wr / (best * 1e-3),
                "of_calibrated_write": wr / (best * 1e-3) / cal,
                "insert_ms": [round(m, 3) for m, _ in ins_ms],
                "insert_keys_per_s": N / (ins_best * 1e-3),
                "insert_pages": ins_pages,
                "bulk_over_insert": ins_best / best,
            })
            print(f"2^{lg} bulk {lf}/{inf}: {best:.3f} ms", flush=True)
        t.close()
        del gen, ids2, sk, sv
    res = {"tool": "tools/bulk_rate.py", "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "insert_runs": args.insert_runs,
           "calibrated_write_GB_per_s": cal / 1e9,
           "calibration": "device fill of %d bytes, best of 5, same process" % args.cal_bytes,
           "bytes_are": "algorithmic: 1088 B per leaf + 1024 B per internal page written; "
                        "16 B per pair read by the check and 16 B by the leaves",
           "times_are": "device events around the call; bulk_load waits for the check's "
                        "status before it writes and for the tree before it returns",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"{'keys':>5} {'fill':>6} {'ms':>8} {'Mkeys/s':>9} {'B/key wr':>8} {'GB/s wr':>8} "
          f"{'of cal.':>7} {'spread':>7} {'insert ms':>10} {'x insert':>8}")
    for r in rows:
        print(f"2^{r['log2_keys']:<3} {r['leaf_fill']:>3}/{r['internal_fill']:<2} "
              f"{min(r['bulk_ms']):>8.3f} {r['keys_per_s'] / 1e6:>9.1f} "
              f"{r['written_bytes_per_key']:>8.2f} {r['written_bytes_per_s'] / 1e9:>8.1f} "
              f"{r['of_calibrated_write']:>7.2f} {r['spread']:>7.3f} "
              f"{min(r['insert_ms']):>10.1f} {r['bulk_over_insert']:>8.1f}")


if __name__ == "__main__":
    main()
