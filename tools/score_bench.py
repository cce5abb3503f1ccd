"""Score (SPEC.md §3 "Score"): LookupTable.score against the path it replaces, on one MI355X.  Numbers go to profiles/score.md.

Per shape the paths take turns inside ONE timing loop, in chunks of 5 calls between device events; the whole sequence runs twice and the spread of a
row is its pass-to-pass difference (the method of tools/search_bench.py).  Same table, same queries, same slates (present ids with `--absent` of them
replaced by ids the table does not hold); score and find write into preallocated buffers, the einsum path allocates its casts and its result.
    score             table.score(queries, keys): probe, row gather and dot product in one launch
    find + einsum     table.find(keys) into a [Q, C, dim] fp32 block, then torch.einsum on the bf16-rounded operands: what a user ran before
    find              the find of that path alone, n = Q * C: the yardstick — the same probe and gather with a larger store
Byte model per candidate: 8 B key + 128 B bucket line + the row + what is stored (score: 4 B; find: a dim * 4 B row).
--metric cosine adds the row `cosine`, table.score(..., metric="cosine"), beside the inner-product rows (profiles/score.md "Metric").
usage: python tools/score_bench.py [--metric ip|cosine] [--keys N] [--dim D] [--reps K] [--shapes 1x1000,256x100,...] [--absent 0.1]"""
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
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--shapes", default="1x1000,256x100,4096x100,256x1000")
ap.add_argument("--metric", default="ip", choices=["ip", "cosine"])
ap.add_argument("--absent", type=float, default=0.1)
args = ap.parse_args()
dev = torch.device("cuda", 0)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


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
    live = t.export()[0]
    row_bytes = args.dim * (4 if value_dtype == torch.float32 else 2)
    for nq, nc in [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(nq * 100003 + nc)
        queries = torch.randn(nq, args.dim, device=dev, generator=gen)
        keys = live[torch.randint(0, live.numel(), (nq, nc), device=dev, generator=gen)]
        miss = torch.rand(nq, nc, device=dev, generator=gen) < args.absent
        keys = torch.where(miss, torch.randint(1 << 62, (1 << 63) - 1, (nq, nc), device=dev, generator=gen), keys).contiguous()
        qb = queries.to(torch.bfloat16).float()
        scores, sfound = torch.empty(nq, nc, device=dev), torch.empty(nq, nc, dtype=torch.uint8, device=dev)
        block, ffound = torch.empty(nq * nc, args.dim, device=dev), torch.empty(nq * nc, dtype=torch.uint8, device=dev)

        def find_einsum():
            t.find(keys, out=block, found=ffound)
            return torch.einsum("qd,qcd->qc", qb, block.view(nq, nc, args.dim).to(torch.bfloat16).float())

        t.score(queries, keys, out=scores, found=sfound)
        hit = sfound.bool()
        assert torch.equal(hit.view(-1), t.find(keys, out=block, found=ffound)[1].bool()) and torch.isneginf(scores[~hit]).all()
        err = float((scores[hit] - find_einsum()[hit]).abs().max()) if hit.any() else 0.0   # (two fp32 summation orders)
        rows = {"score": lambda: t.score(queries, keys, out=scores, found=sfound), "find + einsum": find_einsum,
                "find": lambda: t.find(keys, out=block, found=ffound)}
        if args.metric == "cosine":
            rows["cosine"] = lambda: t.score(queries, keys, out=scores, found=sfound, metric="cosine")
        passes = [timed_rows(rows, args.reps) for _ in range(2)]
        us = {nm: (passes[0][nm] + passes[1][nm]) / 2 for nm in rows}
        n = nq * nc
        score_bytes, find_bytes = n * (8 + 128 + row_bytes + 4), n * (8 + 128 + row_bytes + 4 * args.dim)
        rate = {"score": score_bytes / us["score"] * 1e-6, "find": find_bytes / us["find"] * 1e-6}   # TB/s
        rec = {"metric": args.metric, "rows": str(value_dtype).split(".")[1], "keys": t.size(), "dim": args.dim, "Q": nq, "C": nc, "absent": round(float(miss.float().mean()), 3),
               "us": {nm: round(v, 1) for nm, v in us.items()}, "spread_us": {nm: round(abs(passes[0][nm] - passes[1][nm]), 1) for nm in rows},
               "speedup_over_find_einsum": round(us["find + einsum"] / us["score"], 2), "bytes_per_candidate": {"score": score_bytes // n, "find": find_bytes // n},
               "TBps": {nm: round(v, 3) for nm, v in rate.items()}, "score_rate_over_find_rate": round(rate["score"] / rate["find"], 2),
               "max_abs_diff_to_einsum": err}
        print("SCORE_BENCH " + json.dumps(rec), flush=True)
        results.append(rec)
    del live
    t.close()
    torch.cuda.empty_cache()
print("SCORE_BENCH_ALL " + json.dumps(results), flush=True)
