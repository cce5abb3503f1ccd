"""Search (SPEC.md §3 "Search"): LookupTable.search against what a user ran before it, on one MI355X.  Numbers go to profiles/search.md.

Per shape the two paths take turns inside ONE timing loop, in chunks of 5 calls between device events; the whole sequence runs twice and the spread of
a row is its pass-to-pass difference (the method of profiles/int8_rows.md).
    search            table.search(queries, k): the scan of the table in place and the merge, chunked by the per-call limits where Q * k asks for it
    matmul + topk     on a PREBUILT [N, dim] bf16 matrix of the same table: queries.bfloat16() @ M.T, torch.topk, keys[positions]
    refresh           building that matrix — export() and the cast to bf16 — timed once and reported apart: the cost the matrix path pays after every
                      publish, and the second copy of the table it keeps
usage: python tools/search_bench.py [--keys N] [--dim D] [--reps K] [--queries 1,32,128] [--ks 10,64]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import LookupTable, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--queries", default="1,32,128")
ap.add_argument("--ks", default="10,64", help="one Q and one k: a shape on its own for `rocprofv3 --kernel-trace --stats`, which times the scan and the merge apart")
args = ap.parse_args()
dev = torch.device("cuda", 0)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
PEAK = 8e12   # bytes / s


def timed_rows(rows, reps, chunk=5):
    names = list(rows)
    for nm in names:
        for _ in range(3):
            rows[nm]()
    torch.cuda.synchronize()
    total = dict.fromkeys(names, 0.0)
    for _ in range(reps // chunk):
        for nm in names:
            ev[0].record()
            for _ in range(chunk):
                rows[nm]()
            ev[1].record()
            torch.cuda.synchronize()
            total[nm] += ev[0].elapsed_time(ev[1]) * 1e3
    return {nm: total[nm] / (reps // chunk * chunk) for nm in names}


results = []
for value_dtype in (torch.float32, torch.bfloat16):
    t = LookupTable(int(args.keys / 0.75), args.dim, device=dev, max_batch=1 << 21, value_dtype=value_dtype)
    bench.populate(t, synth, args.keys, args.dim, dev, 1 << 20)
    n = t.size()
    row_bytes = args.dim * (4 if value_dtype == torch.float32 else 2)
    scan_bytes = t.capacity * 8 + n * row_bytes   # what the scan asks for: the key plane and the live rows
    torch.cuda.synchronize()
    ev[0].record()
    ekeys, erows = t.export()[:2]
    matrix = erows.to(torch.bfloat16)
    ev[1].record()
    torch.cuda.synchronize()
    refresh_us = ev[0].elapsed_time(ev[1]) * 1e3
    del erows
    for nq in [int(x) for x in args.queries.split(",")]:
        queries = torch.randn(nq, args.dim, device=dev)
        for k in [int(x) for x in args.ks.split(",")]:
            def matmul_topk():
                pos = torch.topk(queries.to(torch.bfloat16) @ matrix.T, k, dim=1).indices
                return ekeys[pos]

            got = t.search(queries, k)[0]
            same = float((got == matmul_topk()).float().mean())   # (bf16 scores of the matrix path round differently: near-ties may swap)
            rows = {"search": lambda: t.search(queries, k), "matmul + topk": matmul_topk}
            passes = [timed_rows(rows, args.reps) for _ in range(2)]
            us = {nm: (passes[0][nm] + passes[1][nm]) / 2 for nm in rows}
            per_call = min(1536 // max(k, 8), 12288 // args.dim // 32 * 32)
            calls = -(-nq // per_call)
            rec = {"rows": str(value_dtype).split(".")[1], "keys": n, "dim": args.dim, "Q": nq, "k": k, "native_calls": calls,
                   "us": {nm: round(v, 1) for nm, v in us.items()}, "spread_us": {nm: round(abs(passes[0][nm] - passes[1][nm]), 1) for nm in rows},
                   "search_bytes": calls * scan_bytes, "matmul_bytes": n * args.dim * 2 + 2 * nq * n * 2,
                   "search_fraction_of_8TBs": round(calls * scan_bytes / (us["search"] * 1e-6) / PEAK, 3), "refresh_us": round(refresh_us, 1),
                   "refresh_extra_bytes": n * args.dim * 2, "keys_equal_fraction": round(same, 4)}
            print("SEARCH_BENCH " + json.dumps(rec), flush=True)
            results.append(rec)
    del matrix, ekeys
    t.close()
    torch.cuda.empty_cache()
print("SEARCH_BENCH_ALL " + json.dumps(results), flush=True)
