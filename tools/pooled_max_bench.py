"""Max pooling (SPEC.md §3 find_pooled_max / pooled_max_backward) against its neighbours, on one GPU.

Per shape the rows of the table take turns inside ONE timing loop, in chunks of 10 calls between device events, result buffers rotating; the whole
sequence runs twice and the spread of a row is its pass-to-pass difference (the method of profiles/int8_rows.md).
    max + argmax     find_pooled_max with the argmax block (what a training forward runs)
    max              find_pooled_max without it (a serving call)
    sum              find_pooled("sum") on the same inputs: the same bytes read, 4 * dim bytes per bag fewer written than max + argmax
    find + segment   what a user ran before: find into [n, dim], then torch.segment_reduce(..., "max")
    max bwd          pooled_max_backward
    weighted bwd     pooled_weighted_backward(want_weight_grads=False): the other backward that writes [n, dim] grads
Shapes: the 26-table x 2048-bag collection of examples/recsys_collection.py (geometric bag lengths, mean 8) over a TableGroup, and one table with 64K bags
of 20, at dim 64 and 128.
usage: python tools/pooled_max_bench.py [--dims 64,128] [--group-keys N] [--reps K]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from meepoembedding_amd import LookupTable, TableGroup, synth

ap = argparse.ArgumentParser()
ap.add_argument("--group-keys", type=int, default=1_000_000, help="keys stored in every table")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--dims", default="64,128")
ap.add_argument("--tables", type=int, default=26)
ap.add_argument("--bags", type=int, default=2048, help="bags per table of the collection")
ap.add_argument("--mean-len", type=int, default=8)
ap.add_argument("--one-table-bags", type=int, default=65536)
ap.add_argument("--one-table-len", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda", 0)
ROT = 4
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def timed_rows(rows, reps):
    names = list(rows)
    for i in range(5):
        for nm in names:
            rows[nm](i)
    torch.cuda.synchronize()
    total, chunk = dict.fromkeys(names, 0.0), 10
    for c in range(reps // chunk):
        for nm in names:
            ev[0].record()
            for i in range(chunk):
                rows[nm](c * chunk + i)
            ev[1].record()
            torch.cuda.synchronize()
            total[nm] += ev[0].elapsed_time(ev[1]) * 1e3
    return {nm: total[nm] / (reps // chunk * chunk) for nm in names}


def run_shape(name, target, dim, lens, n_tables):
    """target: a LookupTable (n_tables = 1) or a TableGroup; lens: the length of every bag, member-major"""
    off_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, nb = int(off_np[-1]), lens.size
    gen = torch.Generator(device=dev).manual_seed(nb)
    keys = synth.keys_t(1, 0, args.group_keys, dev)[torch.randint(0, args.group_keys, (n,), device=dev, generator=gen)].contiguous()
    off = torch.from_numpy(off_np).to(dev)
    lens_t = torch.from_numpy(np.asarray(lens, np.int64)).to(dev)
    member_off = off[::nb // n_tables].contiguous()
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    outs = [torch.empty((nb, dim), device=dev) for _ in range(ROT)]
    args_ = [torch.empty((nb, dim), dtype=torch.int32, device=dev) for _ in range(ROT)]
    rows_buf = [torch.empty((n, dim), device=dev) for _ in range(2)]
    grads = [torch.empty((n, dim), device=dev) for _ in range(2)]
    bag_grads = torch.randn((nb, dim), device=dev) * 1e-3
    ones = torch.ones(n, device=dev)
    find = (lambda i: target.find(keys, member_off, out=rows_buf[i % 2], found=found)) if n_tables > 1 else (lambda i: target.find(keys, out=rows_buf[i % 2], found=found))

    def composed(i):
        find(i)
        return torch.segment_reduce(rows_buf[i % 2], "max", lengths=lens_t, axis=0, unsafe=True)

    # the rows agree where torch's reduction is defined like ours (bags with keys, no NaN in these tables)
    got = target.find_pooled_max(keys, off, out=outs[0], found=found, argmax=args_[0])[0]
    ref = composed(0)
    torch.cuda.synchronize()
    live = lens_t > 0
    assert torch.equal(got[live], ref[live]), "find_pooled_max differs from find + segment maximum"
    rows = {
        "max + argmax": lambda i: target.find_pooled_max(keys, off, out=outs[i % ROT], found=found, argmax=args_[i % ROT]),
        "max": lambda i: target.find_pooled_max(keys, off, out=outs[i % ROT], found=found),
        "sum": lambda i: target.find_pooled(keys, off, "sum", out=outs[i % ROT], found=found),
        "find + segment": composed,
        "max bwd": lambda i: target.pooled_max_backward(off, args_[0], bag_grads, n, grads=grads[i % 2]),
        "weighted bwd": lambda i: target.pooled_weighted_backward(keys, off, ones, bag_grads, want_weight_grads=False, grads=grads[i % 2]),
    }
    passes = [timed_rows(rows, args.reps) for _ in range(2)]
    rec = {"shape": name, "dim": dim, "n": n, "bags": nb, "wave_per_bag": bool(n // nb >= 12),
           "us": {k: round((passes[0][k] + passes[1][k]) / 2, 2) for k in rows}, "spread_us": {k: round(abs(passes[0][k] - passes[1][k]), 2) for k in rows}}
    print("POOLED_MAX_BENCH " + json.dumps(rec), flush=True)
    return rec


results = []
for dim in [int(d) for d in args.dims.split(",")]:
    tables = []
    for _ in range(args.tables):
        t = LookupTable(int(args.group_keys / 0.75), dim, device=dev, max_batch=1 << 21)
        bench.populate(t, synth, args.group_keys, dim, dev, 1 << 20)
        tables.append(t)
    group = TableGroup(tables)
    rng = np.random.default_rng(dim)
    results.append(run_shape(f"collection {args.tables} x {args.bags} bags, mean {args.mean_len}", group, dim,
                             rng.geometric(1.0 / (args.mean_len + 1), args.tables * args.bags) - 1, args.tables))
    results.append(run_shape(f"one table, {args.one_table_bags} bags of {args.one_table_len}", tables[0], dim,
                             np.full(args.one_table_bags, args.one_table_len), 1))
    group.close()
    for t in tables:
        t.close()
    torch.cuda.empty_cache()
print("POOLED_MAX_BENCH_ALL " + json.dumps(results), flush=True)
