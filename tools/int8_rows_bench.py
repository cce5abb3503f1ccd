"""int8 ROW storage against bf16 and fp32 row storage (SPEC.md §3 "Row storage type"): find on an int8-row table, on a bf16-row table and on
the fp32 table with the same keys.  (An int8-row table has no pooled lookup, so there is no pooled row here.)

Per shape, key distribution and batch the three storage types take turns inside ONE timing loop, in chunks of 10 calls, each row's calls
between device events of its own, result buffers rotating as in the headline of bench.py:
  fp32 / bf16 / int8 rows -> fp32     find
  fp32 / bf16 / int8 rows -> bf16     find(out_dtype=bf16)
The whole sequence runs twice; the spread of a comparison = the largest pass-to-pass difference of the rows compared.  No bar is set: every
int8 figure is reported against the bf16-row and the fp32-row figure of the same run, with that spread, and whether it is faster beyond it.
usage: python tools/int8_rows_bench.py [--keys N] [--small-keys N] [--reps K] [--only big|small]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import LookupTable, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=100_000_000)
ap.add_argument("--small-keys", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--only", choices=["big", "small"])
args = ap.parse_args()
dev = torch.device("cuda", 0)
BF16, ROT = torch.bfloat16, 6
KINDS = (("fp32", {}), ("bf16", dict(value_dtype=BF16)), ("int8", dict(int8_rows=True)))
e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
results = {}


def timed_rows(rows, reps):
    """rows: {name: fn(i)}; the rows take turns in chunks of 10 calls inside one loop -> us per call"""
    names = list(rows)
    for i in range(10):
        for nm in names:
            rows[nm](i)
    torch.cuda.synchronize()
    total = dict.fromkeys(names, 0.0)
    chunk = 10
    for c in range(reps // chunk):
        for nm in names:
            e[0].record()
            for i in range(chunk):
                rows[nm](c * chunk + i)
            e[1].record()
            torch.cuda.synchronize()
            total[nm] += e[0].elapsed_time(e[1]) * 1e3
    return {nm: total[nm] / (reps // chunk * chunk) for nm in names}


def row_bytes(kind, dim):
    return {"fp32": 4 * dim, "bf16": 2 * dim, "int8": dim + 16}[kind]


def find_rows(tabs, dim, batch, n_keys, dist):
    batches = bench.lookup_batches(synth, n_keys, batch, 8, dist, dev, seed=3)
    o32 = [torch.empty((batch, dim), device=dev) for _ in range(ROT)]
    o16 = [torch.empty((batch, dim), dtype=BF16, device=dev) for _ in range(ROT)]
    found = torch.empty(batch, dtype=torch.uint8, device=dev)
    rows, nbytes = {}, {}
    for out_name, outs, out_dtype, out_b in (("fp32", o32, torch.float32, 4 * dim), ("bf16", o16, BF16, 2 * dim)):
        for kind, _ in KINDS:
            t = tabs[kind]
            rows[f"{kind} rows -> {out_name}"] = lambda i, t=t, outs=outs, out_dtype=out_dtype: t.find(batches[i % 8], out=outs[i % ROT], found=found, out_dtype=out_dtype)
            # algorithmic bytes per key: key 8 + bucket line 128 + row + result row (+ found byte, not counted)
            nbytes[f"{kind} rows -> {out_name}"] = 136 + row_bytes(kind, dim) + out_b
    us = timed_rows(rows, args.reps)
    row = {nm: {"us": round(v, 2), "bytes_per_key": nbytes[nm], "TBps": round(nbytes[nm] * batch / v / 1e6, 3)} for nm, v in us.items()}
    shape = f"find dim {dim} batch {batch} {dist}"
    results.setdefault(shape, []).append(row)
    print(shape, json.dumps(row), flush=True)


shapes = [s for s in (("big", args.keys, 64), ("small", args.small_keys, 128)) if args.only in (None, s[0])]
tables = {}
for name, n_keys, dim in shapes:
    tabs = {}
    for kind, kw in KINDS:
        tabs[kind] = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=1 << 20, **kw)
        bench.populate(tabs[kind], synth, n_keys, dim, dev, 1 << 20)
    tables[name] = tabs
    print(f"{name}: {n_keys} keys dim {dim} load 0.75: table_bytes " + ", ".join(f"{k} rows {t.table_bytes} ({t.table_bytes / 1e9:.2f} GB)" for k, t in tabs.items())
          + "; workspace_bytes " + " / ".join(str(t.workspace_bytes) for t in tabs.values()), flush=True)
print(f"{ROT} rotating result buffers; {args.reps} timed calls per row and pass", flush=True)
for p in range(2):
    print(f"--- pass {p + 1}", flush=True)
    for name, n_keys, dim in shapes:
        for dist in ("uniform", "zipf"):
            for batch in (1 << 18, 1 << 20):
                find_rows(tables[name], dim, batch, n_keys, dist)
summary = {}
for shape, (a, b) in results.items():
    out = {"pass1": a, "pass2": b}
    for o in ("fp32", "bf16"):
        i8, others = f"int8 rows -> {o}", (f"bf16 rows -> {o}", f"fp32 rows -> {o}")
        mean = {nm: (a[nm]["us"] + b[nm]["us"]) / 2 for nm in (i8,) + others}
        for other in others:
            spread = max(abs(a[i8]["us"] - b[i8]["us"]), abs(a[other]["us"] - b[other]["us"]))
            out[f"{i8} vs {other}"] = {"int8_us": round(mean[i8], 2), "other_us": round(mean[other], 2), "speedup": round(mean[other] / mean[i8], 3),
                                       "spread_us": round(spread, 2), "faster_beyond_spread": mean[i8] < mean[other] - spread,
                                       "slower_beyond_spread": mean[i8] > mean[other] + spread}
    summary[shape] = out
print("INT8_ROWS_BENCH " + json.dumps(summary), flush=True)
