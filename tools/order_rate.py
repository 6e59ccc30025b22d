#!/usr/bin/env python3
"""Rate of the order statistics (Tree.rank_batch, count_batch, select_batch)
beside the only other way to the same answers.

Trees timed: 2^k hashed keys (gen_keys 1..N, values 2 * id) for k in
--log2-keys (24, 26), each made by bulk_load at 36/40 and by insert_batch
chunks of 2^20 in generation order, whose pages lie in arbitrary order.

Per tree and call: a batch of 2^--log2-batch (20) queries -- keys: half stored,
half random; ranks: random below N; ranges: a stored key and the stored key
--range-keys (1000) positions further -- timed by device events around the
call, the best of --runs after a warm-up with the order index valid, and the
best of --rebuild-runs with the index made stale before each (one pair
written again), which adds the whole-tree count pass and the copy.  rank is
checked against a searchsorted of the sorted keys, select against the sorted
pairs, count against the positions the ranges were drawn from.

Yardsticks, same process and tree: rank as count(0, k - 1) per key on
--rank-sample keys (the per-key mean, scaled to the batch); count as
shm_range_query with offsets = NULL over the same ranges; select as one
scan_batch(0, limit = r + 1) on a tree of 2^--scan-log2 (20) keys for
--select-sample ranks (the mean).

Requests: a query reads one 128 B line per search level (two 64 B requests),
the unit's page, bound and off words (three), and a leaf of 768 or 1024 B (12
or 16); count searches twice and reads two leaves when its ends lie in
different units.  The rate of these requests is set beside the random-request
ceiling of profiles/cal_fetch.json.  The upper levels are small and stay in
L2, so the count is an upper bound on what reaches HBM.

There is no fallback: without a GPU the tool fails.  Writes --out
(profiles/order_rate.json) and prints the table.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP = -(1 << 63)  # unsigned order: flip the top bit around a signed compare
FAN = 16          # order.hip kOrdFan


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log2-keys", type=int, nargs="+", default=[24, 26])
    ap.add_argument("--log2-batch", type=int, default=20)
    ap.add_argument("--range-keys", type=int, default=1000)
    ap.add_argument("--scan-log2", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rebuild-runs", type=int, default=2)
    ap.add_argument("--rank-sample", type=int, default=32)
    ap.add_argument("--select-sample", type=int, default=3)
    ap.add_argument("--no-inserts", action="store_true", help="bulk-loaded trees only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_rate.json"))
    a = ap.parse_args(argv)
    if a.runs < 1 or a.rebuild_runs < 1 or min(a.log2_keys + [a.scan_log2]) < 10:
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


def hashed(torch, t, N):
    gen = torch.empty(N, dtype=torch.int64, device="cuda")
    for first in range(0, N, 1 << 22):
        m = min(1 << 22, N - first)
        t.gen_keys(first + 1, m, gen[first:first + m])
    ids2 = torch.arange(1, N + 1, dtype=torch.int64, device="cuda") * 2
    return gen, ids2


def usorted(torch, gen, ids2):
    sk, order = torch.sort(gen ^ TOP)
    sk ^= TOP
    return sk, ids2[order]


def levels(units):
    n, lev = units, 1
    while n > FAN:
        n = (n + FAN - 1) // FAN
        lev += 1
    return lev


def measure(torch, shm, t, sk, sv, args, what, ceiling):
    N, Q = sk.numel(), 1 << args.log2_batch
    g = torch.Generator(device="cuda").manual_seed(1)
    pos = torch.randint(0, N, (Q,), device="cuda", generator=g)
    keys = sk[pos].clone()
    keys[Q // 2:] = torch.randint(-(1 << 63), (1 << 63) - 1, (Q - Q // 2,), device="cuda",
                                  generator=g)
    ranks = torch.randint(0, N, (Q,), device="cuda", generator=g)
    end = torch.clamp(pos + args.range_keys - 1, max=N - 1)
    lo, hi = sk[pos].clone(), sk[end].clone()
    out = torch.empty(Q, dtype=torch.int64, device="cuda")
    ko, vo = torch.empty_like(out), torch.empty_like(out)
    fo = torch.empty(Q, dtype=torch.uint8, device="cuda")
    calls = {
        "rank": lambda: t.rank_batch(keys, out=out),
        "count": lambda: t.count_batch(lo, hi, out=out),
        "select": lambda: t.select_batch(ranks, keys=ko, vals=vo, found=fo),
    }

    def stale():
        t.insert_batch(sk[:1], sv[:1])  # the same pair again: the index is stale

    row = {"tree": what, "log2_keys": N.bit_length() - 1, "batch": Q}
    for name, call in calls.items():
        call()
        valid = [timed(torch, call) for _ in range(args.runs)]
        if name == "rank":
            want = torch.searchsorted(sk ^ TOP, keys ^ TOP)
            assert bool((out == want).all()), (what, name)
        elif name == "count":
            assert bool((out == end - pos + 1).all()), (what, name)
        else:
            assert bool(fo.all()) and bool((ko == sk[ranks]).all()) and bool((vo == sv[ranks]).all())
        rebuilt = []
        for _ in range(args.rebuild_runs):
            stale()
            b = t.order_stats()["builds"]
            rebuilt.append(timed(torch, call))
            assert t.order_stats()["builds"] == b + 1
        row[name] = {"valid_ms": [round(m, 4) for m in valid],
                     "with_rebuild_ms": [round(m, 3) for m in rebuilt],
                     "queries_per_s": Q / (min(valid) * 1e-3)}
    st = t.order_stats()
    lev = levels(st["units"])
    row.update(units=st["units"], index_bytes=st["bytes"], search_levels=lev,
               last_build_ms=round(st["last_build_ms"], 3))
    per = {"rank": 2 * lev + 3 + 12, "select": 2 * lev + 3 + 12, "count": 2 * (2 * lev + 3 + 12)}
    for name in calls:
        r = row[name]
        r["requests_per_query_at_most"] = per[name]
        r["G_requests_per_s"] = per[name] * r["queries_per_s"] / 1e9
        r["of_random_request_ceiling"] = r["G_requests_per_s"] / ceiling
    # yardsticks: the parent's ways to the same answers
    sample = keys[:args.rank_sample].cpu().tolist()
    t.count(0, 0)
    ms = sum(timed(torch, lambda k=k: t.count(0, (k & ((1 << 64) - 1)) - 1 if k else 0))
             for k in sample) / len(sample)
    row["rank"]["yardstick"] = {"what": "count(0, k - 1) per key, mean of %d" % len(sample),
                                "ms_per_key": round(ms, 4), "ms_per_batch": round(ms * Q, 1),
                                "ratio": ms * Q / min(row["rank"]["valid_ms"])}
    cnt = torch.empty(Q, dtype=torch.int64, device="cuda")

    def range_counts():
        rc = shm.lib().shm_range_query(t.h, shm._ptr(lo), shm._ptr(hi), Q, shm._ptr(cnt), None,
                                       None, shm._stream_ptr(None))
        assert rc == shm.SHM_OK

    range_counts()
    rq = [timed(torch, range_counts) for _ in range(args.runs)]
    assert bool((cnt == end - pos + 1).all())
    row["count"]["yardstick"] = {"what": "shm_range_query(offsets = NULL), same ranges",
                                 "ms": [round(m, 3) for m in rq],
                                 "ratio": min(rq) / min(row["count"]["valid_ms"])}
    for name in calls:
        r = row[name]
        print(f"{what} {name}: {min(r['valid_ms']):.3f} ms valid, "
              f"{min(r['with_rebuild_ms']):.3f} ms with the rebuild, "
              f"{r['queries_per_s'] / 1e9:.3f} G/s, {r['of_random_request_ceiling']:.2f} of the "
              f"request ceiling; yardstick x{r.get('yardstick', {}).get('ratio', float('nan')):.1f}",
              flush=True)
    return row


def select_yardstick(torch, shm, args):
    """one serial scan from key 0 per rank, on a tree of 2^scan_log2 keys"""
    N = 1 << args.scan_log2
    t = shm.Tree(arena_bytes=max(1 << 30, N * 64), max_batch=1 << 20)
    sk, sv = usorted(torch, *hashed(torch, t, N))
    t.bulk_load(sk, sv)
    g = torch.Generator(device="cuda").manual_seed(2)
    ranks = torch.randint(N // 2, N, (args.select_sample,), device="cuda", generator=g)
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    ko = torch.empty(N, dtype=torch.int64, device="cuda")
    vo = torch.empty(N, dtype=torch.int64, device="cuda")
    ms = []
    for r in ranks.cpu().tolist():
        ms.append(timed(torch, lambda r=r: t.scan_batch(zero, r + 1, keys=ko, vals=vo).check()))
        assert int(ko[r]) == int(sk[r])
    t.select_batch(ranks)
    sel = min(timed(torch, lambda: t.select_batch(ranks)) for _ in range(args.runs))
    t.close()
    return {"what": "scan_batch(0, limit = r + 1) per rank at 2^%d keys, ranks in the upper half"
                    % args.scan_log2,
            "scan_ms_per_rank": [round(m, 2) for m in ms],
            "select_batch_of_%d_ms" % len(ms): round(sel, 4),
            "ratio_per_rank": (sum(ms) / len(ms)) / (sel / len(ms))}


def main(argv=None):
    args = parse(argv)
    import torch

    import sherman_amd as shm

    if not torch.cuda.is_available():
        raise SystemExit("order_rate needs a GPU (no fallback)")
    cal = json.load(open(os.path.join(ROOT, "profiles", "cal_fetch.json")))
    ceiling = cal["random_request_ceiling_G_per_s"]
    rows = []
    for lg in args.log2_keys:
        N = 1 << lg
        t = shm.Tree(arena_bytes=max(1 << 30, N * 64), max_batch=1 << 20)
        gen, ids2 = hashed(torch, t, N)
        sk, sv = usorted(torch, gen, ids2)
        t.bulk_load(sk, sv, 36, 40)
        rows.append(measure(torch, shm, t, sk, sv, args, f"2^{lg} bulk 36/40", ceiling))
        if not args.no_inserts:
            t.bulk_load(sk[:0], sv[:0])
            for c in range(0, N, 1 << 20):
                t.insert_batch(gen[c:c + (1 << 20)], ids2[c:c + (1 << 20)])
            rows.append(measure(torch, shm, t, sk, sv, args, f"2^{lg} built by inserts", ceiling))
        t.close()
        del gen, ids2, sk, sv
    res = {"tool": "tools/order_rate.py", "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "random_request_ceiling_G_per_s": ceiling,
           "ceiling_from": "profiles/cal_fetch.json (64 B requests)",
           "requests_are": "algorithmic and an upper bound: two 64 B requests per search level "
                           "(one 128 B line), three for the unit's words, twelve for a 768 B leaf "
                           "read; count twice that.  No level is staged in LDS; the upper levels "
                           "are a few lines every query reads and stay in L2",
           "times_are": "device events around the whole call, best of the runs after a warm-up; "
                        "with_rebuild: the index made stale before each run",
           "rows": rows, "select_yardstick": select_yardstick(torch, shm, args)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    s = res["select_yardstick"]
    print(f"select yardstick: {s['scan_ms_per_rank']} ms per rank by scan, "
          f"x{s['ratio_per_rank']:.0f} per rank")


if __name__ == "__main__":
    main()
