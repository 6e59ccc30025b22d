#!/usr/bin/env python3
"""Rate of the descending limit scans (Tree.rscan_batch) beside the ascending
ones (Tree.scan_batch) from the same starts on the same tree.

tools/scan_rate.py's protocol: a tree of --keys hashed keys (2^24), batches of
--scans scans (2^20) from uniformly random keys, limit in --limits (1, 10,
100).  Each direction is timed with device events around --steps batches after
--warmup, in --runs runs that alternate the two:

  rscan        rscan_batch: the `limit` keys at or below the start, descending
  scan         scan_batch: the `limit` keys at or after it, ascending

Reported per direction: ms per batch (best run, and the spread of the runs),
scans/s, the ratio of the descending rate to the ascending one, and the
algorithmic 64 B requests per scan: the leaves a scan of that length overlaps
(1 + (m - 1) / f for m consecutive keys at f keys per leaf) at 1 KB = 16
requests each, the start's directory entry, 16 B per pair written, and for the
descending scan one more directory entry per step to the left (the ascending
scan holds its sibling pointer in the page it has just read).

There is no fallback: without a GPU the tool fails.  Writes --out
(profiles/rscan_rate.json) and prints the table.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rscan_rate.json"))
    a = ap.parse_args(argv)
    if a.steps < 1 or a.runs < 1 or a.batches < 1 or min(a.limits) < 1:
        ap.error("steps, runs, batches and limits must be positive")
    return a


def requests_per_scan(pairs, keys_per_leaf, descending):
    """(64 B requests, leaves) of a scan that returns `pairs` consecutive keys."""
    leaves = 1.0 + max(pairs - 1.0, 0.0) / keys_per_leaf
    req = 16.0 * leaves + 1.0 + 16.0 * pairs / 64.0
    if descending:
        req += leaves - 1.0
    return req, leaves


def main(argv=None):
    args = parse(argv)
    import torch

    import sherman_amd as shm

    if not torch.cuda.is_available():
        raise SystemExit("rscan_rate needs a GPU (no fallback)")
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
    rows = []
    for limit in args.limits:
        starts = []
        for _ in range(args.batches):
            s = rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64, endpoint=False)
            starts.append(torch.from_numpy(s.view(np.int64)).to(dev))
        keys = torch.empty((n, limit), dtype=torch.int64, device=dev)
        vals = torch.empty((n, limit), dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.zeros(2, dtype=torch.int64, device=dev)

        def rscan_step(i):
            t.rscan_batch(starts[i % args.batches], limit, keys=keys, vals=vals, counts=counts,
                          status=status)

        def scan_step(i):
            t.scan_batch(starts[i % args.batches], limit, keys=keys, vals=vals, counts=counts,
                         status=status)

        forms = [("rscan", rscan_step), ("scan", scan_step)]
        ms = {name: [] for name, _ in forms}
        per = {}
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
                    per[name] = float(counts.sum().item()) / n
        assert status.cpu().tolist()[1] == 0, status
        up = min(ms["scan"])
        for name, _ in forms:
            best = min(ms[name])
            req, leaves = requests_per_scan(per[name], f, name == "rscan")
            req_up, _ = requests_per_scan(per["scan"], f, False)
            rows.append({
                "limit": limit, "form": name, "ms_per_batch": [round(x, 4) for x in ms[name]],
                "scans_per_s": n / (best * 1e-3), "pairs_per_scan": per[name],
                "leaves_per_scan": leaves, "requests_per_scan": req,
                "requests_over_ascending": req / req_up,
                "rate_over_ascending": up / best,
                "spread": (max(ms[name]) - min(ms[name])) / min(ms[name]),
            })
    res = {"tool": "tools/rscan_rate.py", "device": torch.cuda.get_device_name(0), "keys": N,
           "scans_per_batch": n, "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
           "keys_per_leaf": f, "leaves": st["leaves"],
           "requests_are": "algorithmic 64 B requests: 16 per leaf overlapped + the start's "
                           "directory entry + 16 B per pair written; rscan: + one directory "
                           "entry per step to the left",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"{'limit':>5} {'form':<6} {'ms/batch':>9} {'Mscans/s':>9} {'pairs/scan':>10} "
          f"{'req/scan':>9} {'req ratio':>9} {'rate ratio':>10} {'spread':>7}")
    for r in rows:
        print(f"{r['limit']:>5} {r['form']:<6} {min(r['ms_per_batch']):>9.3f} "
              f"{r['scans_per_s'] / 1e6:>9.1f} {r['pairs_per_scan']:>10.2f} "
              f"{r['requests_per_scan']:>9.2f} {r['requests_over_ascending']:>9.3f} "
              f"{r['rate_over_ascending']:>10.3f} {r['spread']:>7.3f}")
    t.close()


if __name__ == "__main__":
    main()
