"""bf16 ROW storage against fp32 row storage (SPEC.md §3 "Row storage type"): find and find_pooled on a bf16-row table and on the fp32
table with the same keys.

Per shape, key distribution and batch the rows take turns inside ONE timing loop, in chunks of 10 calls, each row's calls between device
events of its own, result buffers rotating as in the headline of bench.py:
  fp32 rows -> bf16     the fp32 table's find(out_dtype=bf16)            (the parent commit's code, unchanged)
  bf16 rows -> bf16     the bf16-row table's find(out_dtype=bf16)        (stored bits out as they came)
  fp32 rows -> fp32     the fp32 table's find
  bf16 rows -> fp32     the bf16-row table's find                        (widened in registers)
  pooled fp32 rows / pooled bf16 rows     find_pooled(sum), mean bag length 8, fp32 bag rows
The whole sequence runs twice; the spread of a shape = the larger pass-to-pass difference of the two rows compared.  The condition: the
bf16-row lookup is not slower than the fp32-row lookup of the same shape and output type by more than that spread.
usage: python tools/bf16_rows_bench.py [--keys N] [--small-keys N] [--reps K] [--only big|small]"""
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


def report(shape, us, bytes_per_key, n):
    row = {nm: {"us": round(v, 2), "bytes_per_key": round(bytes_per_key[nm], 1), "TBps": round(bytes_per_key[nm] * n / v / 1e6, 3)} for nm, v in us.items()}
    results.setdefault(shape, []).append(row)
    print(shape, json.dumps(row), flush=True)


def find_rows(tf, tb, dim, batch, n_keys, dist):
    batches = bench.lookup_batches(synth, n_keys, batch, 8, dist, dev, seed=3)
    o32 = [torch.empty((batch, dim), device=dev) for _ in range(ROT)]
    o16 = [torch.empty((batch, dim), dtype=BF16, device=dev) for _ in range(ROT)]
    found = torch.empty(batch, dtype=torch.uint8, device=dev)
    rows = {"fp32 rows -> bf16": lambda i: tf.find(batches[i % 8], out=o16[i % ROT], found=found, out_dtype=BF16),
            "bf16 rows -> bf16": lambda i: tb.find(batches[i % 8], out=o16[i % ROT], found=found, out_dtype=BF16),
            "fp32 rows -> fp32": lambda i: tf.find(batches[i % 8], out=o32[i % ROT], found=found),
            "bf16 rows -> fp32": lambda i: tb.find(batches[i % 8], out=o32[i % ROT], found=found)}
    # algorithmic bytes per key: key 8 + bucket line 128 + row + result row (+ found byte, not counted)
    b = {"fp32 rows -> bf16": 136 + 4 * dim + 2 * dim, "bf16 rows -> bf16": 136 + 2 * dim + 2 * dim,
         "fp32 rows -> fp32": 136 + 4 * dim + 4 * dim, "bf16 rows -> fp32": 136 + 2 * dim + 4 * dim}
    report(f"find dim {dim} batch {batch} {dist}", timed_rows(rows, args.reps), b, batch)


def pooled_rows(tf, tb, dim, batch, n_keys, dist):
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    lens = torch.randint(1, 16, (batch // 8,), device=dev, generator=g)   # bag lengths 1-15, mean 8
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    n, nb = int(off[-1]), lens.numel()
    keys = [b[:n].contiguous() for b in bench.lookup_batches(synth, n_keys, batch + 4096, 8, dist, dev, seed=6)]
    o32 = [torch.empty((nb, dim), device=dev) for _ in range(ROT)]
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    rows = {"pooled fp32 rows": lambda i: tf.find_pooled(keys[i % 8], off, "sum", out=o32[i % ROT], found=found),
            "pooled bf16 rows": lambda i: tb.find_pooled(keys[i % 8], off, "sum", out=o32[i % ROT], found=found)}
    L = n / nb
    b = {"pooled fp32 rows": 136 + 4 * dim + 4 * dim / L, "pooled bf16 rows": 136 + 2 * dim + 4 * dim / L}
    report(f"find_pooled sum dim {dim}, {nb} bags of 1-15 keys ({n} keys) {dist}", timed_rows(rows, args.reps), b, n)


shapes = [s for s in (("big", args.keys, 64), ("small", args.small_keys, 128)) if args.only in (None, s[0])]
tables = {}
for name, n_keys, dim in shapes:
    tf = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=1 << 20)
    tb = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=1 << 20, value_dtype=BF16)
    bench.populate(tf, synth, n_keys, dim, dev, 1 << 20)
    bench.populate(tb, synth, n_keys, dim, dev, 1 << 20)
    tables[name] = (tf, tb)
    print(f"{name}: {n_keys} keys dim {dim} load 0.75: table_bytes fp32 rows {tf.table_bytes} ({tf.table_bytes / 1e9:.2f} GB), bf16 rows {tb.table_bytes} "
          f"({tb.table_bytes / 1e9:.2f} GB); workspace_bytes {tf.workspace_bytes} / {tb.workspace_bytes}", flush=True)
print(f"{ROT} rotating result buffers; {args.reps} timed calls per row and pass", flush=True)
for p in range(2):
    print(f"--- pass {p + 1}", flush=True)
    for name, n_keys, dim in shapes:
        tf, tb = tables[name]
        for dist in ("uniform", "zipf"):
            for batch in (1 << 18, 1 << 20):
                find_rows(tf, tb, dim, batch, n_keys, dist)
            pooled_rows(tf, tb, dim, 1 << 18, n_keys, dist)
summary = {}
PAIRS = (("fp32 rows -> bf16", "bf16 rows -> bf16"), ("fp32 rows -> fp32", "bf16 rows -> fp32"), ("pooled fp32 rows", "pooled bf16 rows"))
for shape, (a, b) in results.items():
    out = {"pass1": a, "pass2": b}
    for f, h in PAIRS:
        if f in a:
            spread = max(abs(a[f]["us"] - b[f]["us"]), abs(a[h]["us"] - b[h]["us"]))
            mf, mh = (a[f]["us"] + b[f]["us"]) / 2, (a[h]["us"] + b[h]["us"]) / 2
            out[h] = {"fp32_rows_us": round(mf, 2), "bf16_rows_us": round(mh, 2), "speedup": round(mf / mh, 3), "spread_us": round(spread, 2),
                      "not_slower_beyond_spread": mh <= mf + spread}
    summary[shape] = out
print("BF16_ROWS_BENCH " + json.dumps(summary), flush=True)
