#!/usr/bin/env python3
"""Rate of the ordered limit scans (Tree.scan_batch) beside the unordered
slot scans of the same expected length (Tree.range_query_slots).

Workload: a tree of --keys hashed keys (2^24), batches of --scans scans
(2^20) from uniformly random keys, limit in --limits (1, 10, 100).  Each scan
form is timed with device events around --steps batches after --warmup, in
--runs runs that alternate the forms:

  scan         scan_batch
  slots        range_query_slots over the windows [from, from + limit * 2^64 /
               N] with slot_cap = 4 * limit: the same expected length,
               values only, in leaf / slot order

Reported per form: scans/s, output pairs/s (values/s for slots), and the
algorithmic HBM bytes per scan -- the leaves a scan of that length overlaps
(1 + (m - 1) / f for m consecutive keys at f keys per leaf; a window of width
W holds W / w leaves more than one, w a leaf's key width) at 1 KB each plus
16 B per pair written (8 B per value for slots) -- as 64 B requests per
second against the calibrated random-request rate in profiles/cal_fetch.json.

There is no fallback: without a GPU the tool fails.  Writes --out
(profiles/scan_rate.json) and prints the table.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U64 = np.uint64


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--keys", type=int, default=1 << 24)
    ap.add_argument("--scans", type=int, default=1 << 20)
    ap.add_argument("--limits", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4, help="distinct scan batches, rotated")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_rate.json"))
    a = ap.parse_args(argv)
    if a.steps < 1 or a.runs < 1 or a.batches < 1 or min(a.limits) < 1:
        ap.error("steps, runs, batches and limits must be positive")
    return a


def calibrated_requests_per_s():
    """The random 64 B request rate of profiles/cal_fetch.json (the best kernel)."""
    cal = json.load(open(os.path.join(ROOT, "profiles", "cal_fetch.json")))
    return max(k["G_requests_per_s"] for k in cal["kernels"]) * 1e9


def window_width(limit, n_keys):
    """Key width that holds `limit` of n_keys uniformly spread keys."""
    return (limit << 64) // n_keys


def scan_bytes(pairs_per_scan, keys_per_leaf, word_bytes):
    """Algorithmic bytes of a scan that returns pairs_per_scan consecutive
    keys: the leaves it overlaps at 1 KB each + what it writes."""
    leaves = 1.0 + max(pairs_per_scan - 1.0, 0.0) / keys_per_leaf
    return 1024.0 * leaves + word_bytes * pairs_per_scan, leaves


def main(argv=None):
    args = parse(argv)
    import torch

    import sherman_amd as shm

    if not torch.cuda.is_available():
        raise SystemExit("scan_rate needs a GPU (no fallback)")
    dev = "cuda"
    N, n = args.keys, args.scans
    t = shm.Tree(arena_bytes=max(1 << 30, N * 64), max_batch=1 << 20)
    kb = torch.empty(1 << 20, dtype=torch.int64, device=dev)
    for first in range(1, N + 1, 1 << 20):
        m = min(1 << 20, N + 1 - first)
        t.gen_keys(first, m, kb[:m])
        t.insert_batch(kb[:m], kb[:m] ^ 0x5A5A)
    st = t.check()
    assert st["keys"] == N, st
    f = st["keys"] / st["leaves"]
    rng = np.random.default_rng(args.seed)
    stream = torch.cuda.current_stream()
    cal = calibrated_requests_per_s()
    rows = []
    for limit in args.limits:
        W = window_width(limit, N)
        cap = 4 * limit
        los, his = [], []
        for _ in range(args.batches):
            lo = rng.integers(0, (1 << 64) - W, n, dtype=np.uint64, endpoint=False)
            los.append(torch.from_numpy(lo.view(np.int64)).to(dev))
            his.append(torch.from_numpy((lo + U64(W)).view(np.int64)).to(dev))
        keys = torch.empty((n, limit), dtype=torch.int64, device=dev)
        vals = torch.empty((n, limit), dtype=torch.int64, device=dev)
        svals = torch.empty((n, cap), dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.zeros(2, dtype=torch.int64, device=dev)

        def scan_step(i):
            t.scan_batch(los[i % args.batches], limit, keys=keys, vals=vals, counts=counts,
                         status=status)

        def slots_step(i):
            t.range_query_slots(los[i % args.batches], his[i % args.batches], cap, vals=svals,
                                counts=counts, status=status)

        forms = [("scan", scan_step), ("slots", slots_step)]
        ms = {name: [] for name, _ in forms}
        out = {}
        for run in range(args.runs + 1):  # run 0: warm-up and the counts
            for name, step in forms:
                for i in range(args.warmup):
                    step(i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for i in range(args.steps):
                    step(i)
                e1.record(stream)
                e1.synchronize()
                t.synchronize()
                if run:
                    ms[name].append(e0.elapsed_time(e1) / args.steps)
                else:
                    c = counts.clamp(max=cap if name == "slots" else limit)
                    out[name] = float(c.sum().item()) / n
        assert status.cpu().tolist()[1] == 0, status
        for name, _ in forms:
            per = out[name]
            nbytes, leaves = scan_bytes(per, f, 8.0 if name == "slots" else 16.0)
            if name == "slots":  # a key window overlaps one leaf more than its width in leaves
                leaves = 1.0 + per / f
                nbytes = 1024.0 * leaves + 8.0 * per
            best = min(ms[name])
            rows.append({
                "limit": limit, "form": name, "ms_per_batch": [round(x, 4) for x in ms[name]],
                "scans_per_s": n / (best * 1e-3), "pairs_per_scan": per,
                "pairs_per_s": per * n / (best * 1e-3), "leaves_per_scan": leaves,
                "bytes_per_scan": nbytes,
                "requests_per_s": nbytes / 64.0 * n / (best * 1e-3),
                "of_calibrated_requests": nbytes / 64.0 * n / (best * 1e-3) / cal,
                "spread": (max(ms[name]) - min(ms[name])) / min(ms[name]),
            })
    res = {"tool": "tools/scan_rate.py", "device": torch.cuda.get_device_name(0), "keys": N,
           "scans_per_batch": n, "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
           "keys_per_leaf": f, "leaves": st["leaves"],
           "calibrated_G_requests_per_s": cal / 1e9,
           "bytes_are": "algorithmic: 1 KB per leaf overlapped + bytes written", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"{'limit':>5} {'form':<11} {'ms/batch':>9} {'Mscans/s':>9} {'pairs/scan':>10} "
          f"{'Mpairs/s':>9} {'B/scan':>7} {'of cal.':>7} {'spread':>7}")
    for r in rows:
        print(f"{r['limit']:>5} {r['form']:<11} {min(r['ms_per_batch']):>9.3f} "
              f"{r['scans_per_s'] / 1e6:>9.1f} {r['pairs_per_scan']:>10.2f} "
              f"{r['pairs_per_s'] / 1e6:>9.1f} {r['bytes_per_scan']:>7.0f} "
              f"{r['of_calibrated_requests']:>7.2f} {r['spread']:>7.3f}")
    t.close()


if __name__ == "__main__":
    main()
