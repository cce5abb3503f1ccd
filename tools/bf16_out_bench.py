"""bf16 output against fp32 output (+ the cast users put behind it): find, the training forward, pooled lookups.

Per shape three rows alternate inside ONE timing loop — 1: the fp32 lookup (the library's default path), 2: the fp32 lookup followed by
rows.to(torch.bfloat16), 3: the bf16 lookup — device events around >= 100 calls each after warm-up, result buffers rotating as in the
headline of bench.py.  The whole sequence runs twice; the spread between the passes is what a difference has to exceed to be one.
usage: python tools/bf16_out_bench.py [--keys N] [--small-keys N] [--fp32-only] [--reps K] [--only headline|dim16]
  --only:      one find triple alone — headline = dim 64, 256K keys on the large table; dim16 = dim 16 on a small one (the runs to put under
               `rocprofv3 --kernel-trace --stats -- python ...`: one shape per kernel name)
  --fp32-only: row 1 alone (what a library without the typed entry points can run: the same tool against the parent commit's build,
               MEE_LIB_PATH=<its libmeepo_hip.so> MEE_LIB_OLDER_BUILD=1)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import OPT_ADAGRAD, LookupTable, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=100_000_000)
ap.add_argument("--small-keys", type=int, default=10_000_000)
ap.add_argument("--fp32-only", action="store_true")
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--only", choices=["headline", "dim16"])
args = ap.parse_args()
dev = torch.device("cuda", 0)
BF16, ROT = torch.bfloat16, 6
e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
results = {}


def timed_rows(rows, reps):
    """rows: {name: fn(i)}; the rows take turns call by call inside one loop, each row's calls timed by events of its own -> us per call"""
    names = list(rows)
    for i in range(10):
        for nm in names:
            rows[nm](i)
    torch.cuda.synchronize()
    total = dict.fromkeys(names, 0.0)
    chunk = 10
    for c in range(reps // chunk):           # alternate in chunks of 10 calls: every row sees the same drift of clocks and cache state
        for nm in names:
            e[0].record()
            for i in range(chunk):
                rows[nm](c * chunk + i)
            e[1].record()
            torch.cuda.synchronize()
            total[nm] += e[0].elapsed_time(e[1]) * 1e3
    return {nm: total[nm] / (reps // chunk * chunk) for nm in names}


def report(shape, us, bytes_per_key, n):
    """bytes_per_key: {row: algorithmic bytes per key}"""
    row = {nm: {"us": round(v, 2), "bytes_per_key": round(bytes_per_key[nm], 1), "TBps": round(bytes_per_key[nm] * n / v / 1e6, 3)} for nm, v in us.items()}
    if "bf16" in us:
        row["ratio_3_to_1"] = round(us["fp32"] / us["bf16"], 3)
        row["ratio_3_to_2"] = round(us["fp32+cast"] / us["bf16"], 3)
    results.setdefault(shape, []).append(row)
    print(shape, json.dumps(row), flush=True)


def find_triple(t, dim, batch, n_keys, tag):
    batches = bench.lookup_batches(synth, n_keys, batch, 8, "uniform", dev, seed=3)
    o32 = [torch.empty((batch, dim), device=dev) for _ in range(ROT)]
    o16 = [torch.empty((batch, dim), dtype=BF16, device=dev) for _ in range(ROT)]
    found = torch.empty(batch, dtype=torch.uint8, device=dev)
    rows = {"fp32": lambda i: t.find(batches[i % 8], out=o32[i % ROT], found=found)}
    if not args.fp32_only:
        rows["fp32+cast"] = lambda i: o16[i % ROT].copy_(t.find(batches[i % 8], out=o32[i % ROT], found=found)[0])
        rows["bf16"] = lambda i: t.find(batches[i % 8], out=o16[i % ROT], found=found, out_dtype=BF16)
    b = {"fp32": 16 + 8 * dim, "fp32+cast": 16 + 8 * dim + 6 * dim, "bf16": 16 + 6 * dim}
    report(f"find dim {dim} batch {batch} {tag}", timed_rows(rows, args.reps), b, batch)


def forward_triple(t, dim, batch, n_keys):
    batches = bench.lookup_batches(synth, n_keys, batch, 8, "uniform", dev, seed=4)
    o32 = [torch.empty((batch, dim), device=dev) for _ in range(ROT)]
    o16 = [torch.empty((batch, dim), dtype=BF16, device=dev) for _ in range(ROT)]
    found, slots = torch.empty(batch, dtype=torch.uint8, device=dev), torch.empty(batch, dtype=torch.int64, device=dev)

    def fwd(i, out, **kw):
        r = t.find_located(batches[i % 8], out=out, found=found, slots=slots, prepare_apply=True, **kw)
        t.apply_discard()
        return r[0]
    rows = {"fp32": lambda i: fwd(i, o32[i % ROT])}
    if not args.fp32_only:
        rows["fp32+cast"] = lambda i: o16[i % ROT].copy_(fwd(i, o32[i % ROT]))
        rows["bf16"] = lambda i: fwd(i, o16[i % ROT], out_dtype=BF16)
    b = {"fp32": 24 + 8 * dim, "fp32+cast": 24 + 8 * dim + 6 * dim, "bf16": 24 + 6 * dim}   # + 8 B handle per key
    report(f"find_located(prepare_apply) + apply_discard dim {dim} batch {batch}", timed_rows(rows, args.reps), b, batch)


def pooled_triple(t, dim, batch, n_keys):
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    lens = torch.randint(1, 41, (batch // 22,), device=dev, generator=g)   # bag lengths 1-40, mean 20.5
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    n, nb = int(off[-1]), lens.numel()
    keys = [b[:n].contiguous() for b in bench.lookup_batches(synth, n_keys, batch + 4096, 8, "uniform", dev, seed=6)]
    o32 = [torch.empty((nb, dim), device=dev) for _ in range(ROT)]
    o16 = [torch.empty((nb, dim), dtype=BF16, device=dev) for _ in range(ROT)]
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    rows = {"fp32": lambda i: t.find_pooled(keys[i % 8], off, "sum", out=o32[i % ROT], found=found)}
    if not args.fp32_only:
        rows["fp32+cast"] = lambda i: o16[i % ROT].copy_(t.find_pooled(keys[i % 8], off, "sum", out=o32[i % ROT], found=found)[0])
        rows["bf16"] = lambda i: t.find_pooled(keys[i % 8], off, "sum", out=o16[i % ROT], found=found, out_dtype=BF16)
    L = n / nb
    b = {"fp32": 16 + 4 * dim + 4 * dim / L, "fp32+cast": 16 + 4 * dim + (4 + 6) * dim / L, "bf16": 16 + 4 * dim + 2 * dim / L}
    report(f"find_pooled sum dim {dim}, {nb} bags of 1-40 keys ({n} keys)", timed_rows(rows, args.reps), b, n)


dims_small = {None: (16, 32, 128), "headline": (), "dim16": (16,)}[args.only]
big = None
if args.only != "dim16":
    big = LookupTable(int(args.keys / 0.75), 64, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 20, initial_accumulator=0.1)
    bench.populate(big, synth, args.keys, 64, dev, 1 << 20)
small = {}
for dim in dims_small:
    small[dim] = LookupTable(int(args.small_keys / 0.75), dim, device=dev, max_batch=1 << 20)
    bench.populate(small[dim], synth, args.small_keys, dim, dev, 1 << 20)
print(f"tables: {args.keys} keys dim 64 (Adagrad planes), {args.small_keys} keys at dims 16 / 32 / 128; load 0.75; {ROT} rotating result buffers; "
      f"{args.reps} timed calls per row and pass" + (f"; only: {args.only}" if args.only else ""), flush=True)
for p in range(2):
    print(f"--- pass {p + 1}", flush=True)
    if big is not None:
        find_triple(big, 64, 1 << 18, args.keys, "(configs[1])")
    if args.only is None:
        find_triple(big, 64, 1 << 20, args.keys, "")
    for dim in dims_small:
        find_triple(small[dim], dim, 1 << 18, args.small_keys, "")
    if args.only is None:
        forward_triple(big, 64, 1 << 18, args.keys)
        pooled_triple(big, 64, 1 << 18, args.keys)
summary = {}
for shape, (a, b) in results.items():
    spread = {nm: round(abs(a[nm]["us"] - b[nm]["us"]), 2) for nm in ("fp32", "fp32+cast", "bf16") if nm in a}
    summary[shape] = {"pass1": a, "pass2": b, "spread_us": spread}
print("BF16_OUT_BENCH " + json.dumps(summary), flush=True)
