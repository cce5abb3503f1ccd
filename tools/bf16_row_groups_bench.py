"""A bf16-row table group against what else can serve a collection (SPEC.md §3 "Row storage type"): the pooled lookup of the collection of
examples/recsys_collection.py — 26 tables of 2 x 10^6 slots holding 10^6 keys each, dim 64, 2048 samples per batch, one bag per (table, sample),
bag lengths 1-15 (mean 8), fp32 bag rows — on uniform and Zipf(1.05) keys.

Per key distribution the rows take turns inside ONE timing loop, in chunks of 10 calls, each row's calls between device events of its own,
result buffers rotating:
  fp32 group, 1 launch         the fp32 TableGroup's find_pooled                              (a)
  bf16-row tables, 26 launches find_pooled on each bf16-row table, what serving cost before   (b)
  bf16-row group, 1 launch     the bf16-row TableGroup's find_pooled                          (c)
The whole sequence runs twice; spread = the larger pass-to-pass difference of the rows compared.  (c) is compared against (a) and (b).
usage: python tools/bf16_row_groups_bench.py [--keys N] [--reps K]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import LookupTable, TableGroup, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=1_000_000, help="keys stored per table (the table has twice as many slots)")
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
dev = torch.device("cuda", 0)
N_TABLES, DIM, BATCH, ROT = 26, 64, 2048, 6
A, B, Cc = "fp32 group, 1 launch", "bf16-row tables, 26 launches", "bf16-row group, 1 launch"
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


def pooled_rows(gf, gb, dist):
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    lens = torch.randint(1, 16, (N_TABLES * BATCH,), device=dev, generator=g)   # bag lengths 1-15, mean 8
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    n, nb = int(off[-1]), lens.numel()
    keys = [b[:n].contiguous() for b in bench.lookup_batches(synth, args.keys, n + 4096, 8, dist, dev, seed=6)]
    # the per-table form of the same request: member j's keys and its bag offsets rebased to them
    bounds = [int(x) for x in off[::BATCH].cpu()]
    seg_keys = [[k[bounds[j]:bounds[j + 1]].contiguous() for j in range(N_TABLES)] for k in keys]
    seg_off = [(off[j * BATCH:(j + 1) * BATCH + 1] - bounds[j]).contiguous() for j in range(N_TABLES)]
    out = [torch.empty((nb, DIM), device=dev) for _ in range(ROT)]
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    seg_found = [found[bounds[j]:bounds[j + 1]] for j in range(N_TABLES)]

    def per_table(i):
        o = out[i % ROT]
        for j, t in enumerate(gb.tables):
            t.find_pooled(seg_keys[i % 8][j], seg_off[j], "sum", out=o[j * BATCH:(j + 1) * BATCH], found=seg_found[j])

    rows = {A: lambda i: gf.find_pooled(keys[i % 8], off, "sum", out=out[i % ROT], found=found),
            B: per_table,
            Cc: lambda i: gb.find_pooled(keys[i % 8], off, "sum", out=out[i % ROT], found=found)}
    a = gf.find_pooled(keys[0], off, "sum")[0]
    per_table(0)
    assert torch.equal(out[0], gb.find_pooled(keys[0], off, "sum")[0])          # (b) and (c) compute the same rows
    assert float((a - out[0]).abs().max()) < 0.05 * float(a.abs().max())        # and (a) the unrounded ones
    L = n / nb
    # algorithmic bytes per key: key 8 + bucket line 128 + row + the key's share of the bag row (+ found byte, not counted)
    bpk = {A: 136 + 4 * DIM + 4 * DIM / L, B: 136 + 2 * DIM + 4 * DIM / L, Cc: 136 + 2 * DIM + 4 * DIM / L}
    us = timed_rows(rows, args.reps)
    row = {nm: {"us": round(v, 2), "bytes_per_key": round(bpk[nm], 1), "TBps": round(bpk[nm] * n / v / 1e6, 3)} for nm, v in us.items()}
    shape = f"find_pooled sum, {N_TABLES} tables x {BATCH} bags of 1-15 keys ({n} keys), dim {DIM}, {dist}"
    results.setdefault(shape, []).append(row)
    print(shape, json.dumps(row), flush=True)


tables = [LookupTable(2 * args.keys, DIM, device=dev, max_batch=1 << 18) for _ in range(N_TABLES)]
for t in tables:
    bench.populate(t, synth, args.keys, DIM, dev, 1 << 18)
gf = TableGroup(tables)
gb = gf.serving_copy()
print(f"{N_TABLES} tables x {args.keys} keys, dim {DIM}, load 0.5: table_bytes fp32 group {sum(t.table_bytes for t in gf.tables)} "
      f"({sum(t.table_bytes for t in gf.tables) / 1e9:.2f} GB), bf16-row group {sum(t.table_bytes for t in gb.tables)} "
      f"({sum(t.table_bytes for t in gb.tables) / 1e9:.2f} GB)", flush=True)
print(f"{ROT} rotating result buffers; {args.reps} timed calls per row and pass", flush=True)
for p in range(2):
    print(f"--- pass {p + 1}", flush=True)
    for dist in ("uniform", "zipf"):
        pooled_rows(gf, gb, dist)
summary = {}
for shape, (a, b) in results.items():
    out = {"pass1": a, "pass2": b}
    mean = {nm: (a[nm]["us"] + b[nm]["us"]) / 2 for nm in a}
    for other, tag in ((A, "vs_fp32_group"), (B, "vs_per_table")):
        spread = max(abs(a[other]["us"] - b[other]["us"]), abs(a[Cc]["us"] - b[Cc]["us"]))
        out[tag] = {"other_us": round(mean[other], 2), "bf16_row_group_us": round(mean[Cc], 2), "speedup": round(mean[other] / mean[Cc], 3),
                    "spread_us": round(spread, 2), "not_slower_beyond_spread": mean[Cc] <= mean[other] + spread}
    summary[shape] = out
print("BF16_ROW_GROUPS_BENCH " + json.dumps(summary), flush=True)
