"""Shared slate (SPEC.md §3 "Score", "Shared slate"): table.score(q, keys [C]) against the only way to get the same block before it,
table.score(q, keys.expand(Q, C).contiguous()) with that [Q, C] block built OUTSIDE the timed region.  Numbers go to profiles/score_shared.md.

Per shape the two paths take turns: one warm-up call each, then `reps` rounds of (shared, per-query), each round 5 calls of a path between two device
events (one call where a call is longer than --slow-ms, and then 3 rounds only); the figure is the median per call.  A call is the Python method,
its checks and the launch: below some 30 us both paths' figures are host and launch overhead as much as kernel time.  The table holds --keys live
rows, so a slate's rows do not all sit in L2.  --shared-only leaves the per-query path out (builds compared through MEE_LIB_PATH).
usage: python tools/score_shared_bench.py [--keys N] [--dims 64,256,1024] [--queries 1,32,256,4096] [--cands 1024,65536] [--reps K] [--metric ip|cosine]
                                          [--rows fp32,bf16] [--shared-only]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import LookupTable, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=1_000_000)
ap.add_argument("--dims", default="64,256,1024")
ap.add_argument("--queries", default="1,32,256,4096")
ap.add_argument("--cands", default="1024,65536")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--slow-ms", type=float, default=20.0)
ap.add_argument("--metric", default="ip", choices=["ip", "cosine"])
ap.add_argument("--rows", default="fp32,bf16")
ap.add_argument("--shared-only", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)


def once(fn, calls=1):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(calls):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / calls


results = []
for dim in (int(d) for d in args.dims.split(",")):
    for value_dtype in [{"fp32": torch.float32, "bf16": torch.bfloat16}[r] for r in args.rows.split(",")]:
        t = LookupTable(int(args.keys / 0.75), dim, device=dev, max_batch=1 << 20, value_dtype=value_dtype)
        bench.populate(t, synth, args.keys, dim, dev, 1 << 18)
        live = t.export()[0]
        for nc in (int(c) for c in args.cands.split(",")):
            for nq in (int(q) for q in args.queries.split(",")):
                gen = torch.Generator(device=dev).manual_seed(nq * 100003 + nc)
                queries = torch.randn(nq, dim, device=dev, generator=gen)
                keys = live[torch.randint(0, live.numel(), (nc,), device=dev, generator=gen)].contiguous()
                keys2d = keys.expand(nq, nc).contiguous()
                out, found = torch.empty(nq, nc, device=dev), torch.empty(nc, dtype=torch.uint8, device=dev)
                out2, found2 = torch.empty(nq, nc, device=dev), torch.empty(nq, nc, dtype=torch.uint8, device=dev)
                paths = {"shared": lambda: t.score(queries, keys, out=out, found=found, metric=args.metric),
                         "per_query": lambda: t.score(queries, keys2d, out=out2, found=found2, metric=args.metric)}
                warm = {nm: once(fn) for nm, fn in paths.items()}
                diff = float((out - out2).abs().nan_to_num(nan=float("inf")).max())   # (two fp32 summation orders; a NaN on one side only shows as inf)
                if args.shared_only:
                    del paths["per_query"]
                slow = max(warm.values()) > args.slow_ms * 1e3
                reps, calls = (3, 1) if slow else (args.reps, 5)
                us = {nm: [] for nm in paths}
                for _ in range(reps):
                    for nm, fn in paths.items():
                        us[nm].append(once(fn, calls))
                med = {nm: statistics.median(v) for nm, v in us.items()}
                rec = {"metric": args.metric, "rows": str(value_dtype).split(".")[1], "keys": t.size(), "dim": dim, "Q": nq, "C": nc, "reps": reps, "calls": calls,
                       "us": {nm: round(v, 1) for nm, v in med.items()}, "min_us": {nm: round(min(v), 1) for nm, v in us.items()},
                       "per_query_over_shared": None if args.shared_only else round(med["per_query"] / med["shared"], 2), "max_abs_diff": diff}
                print("SCORE_SHARED_BENCH " + json.dumps(rec), flush=True)
                results.append(rec)
                del keys2d, out, out2, found2
        del live
        t.close()
        torch.cuda.empty_cache()
print("SCORE_SHARED_BENCH_ALL " + json.dumps(results), flush=True)
