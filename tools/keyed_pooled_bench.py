"""The keyed pooled lookups (SPEC.md §3 "Keyed output") against what a user without them runs for the same [batch, sum of dims] block.

Forward, composition: the table-major launch plus the copy that makes the block — view / transpose / reshape for a uniform group and a group of pairs,
torch.cat(views, 1) for a mixed group.  Forward, keyed: find_pooled(layout="keyed", step_index=) — the launch a training step runs, the step index included.  Two more rows time the table-major
launch alone and the keyed launch without a step index (a serving call): their difference is the store pattern alone.
Backward (fp32, Adagrad, mode "mean"), composition: the permute-back copy of the block's gradient (mixed: the split into the class-major buffer), the
position-to-bag index (arange + repeat_interleave), the mean's division and apply_pooled.  Keyed: the division of the keyed block and apply_pooled through the
emitted index (mixed: apply_pooled(layout="keyed", mean_offsets=), whose one launch takes the gradient apart and divides).
Per shape the rows take turns inside ONE timing loop, in chunks of 10 calls between device events, result blocks rotating; the whole sequence runs twice and
the spread of a comparison is the largest pass-to-pass difference of the two rows compared.
usage: python tools/keyed_pooled_bench.py [--what uniform,tiered,mixed] [--group-keys N] [--reps K] [--bags B] [--tables T]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from meepoembedding_amd import OPT_ADAGRAD, LookupTable, MixedTableGroup, TableGroup, _lib, synth
from meepoembedding_amd.tiered import TieredLookupTable, TieredTableGroup

ap = argparse.ArgumentParser()
ap.add_argument("--group-keys", type=int, default=1_000_000, help="keys in every member (in each tier of every pair)")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--bags", type=int, default=2048, help="bags per table")
ap.add_argument("--tables", type=int, default=26)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--mean-len", type=int, default=8)
ap.add_argument("--what", default="uniform,tiered,mixed")
args = ap.parse_args()
dev = torch.device("cuda", 0)
BF16, ROT = torch.bfloat16, 4
MIXED_DIMS = (8, 64, 128, 64, 8, 128)   # examples/mixed_collection.py
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
results = {}


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


def batch_for(n_tables, n_keys, seed, cold_share=0.0):
    """bag lengths geometric with the given mean, keys uniform over each member's stored keys (cold_share of them from the cold tier's range)"""
    rng = np.random.default_rng(seed)
    lens = rng.geometric(1.0 / (args.mean_len + 1), n_tables * args.bags) - 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    gen = torch.Generator(device=dev).manual_seed(seed)
    keys = synth.keys_t(1, 0, n_keys, dev)[torch.randint(0, n_keys, (n,), device=dev, generator=gen)]
    if cold_share:
        cold_keys = synth.keys_t(1, n_keys, n_keys, dev)[torch.randint(0, n_keys, (n,), device=dev, generator=gen)]
        keys = torch.where(torch.rand(n, device=dev, generator=gen) < cold_share, cold_keys, keys)
    return keys.contiguous(), torch.from_numpy(off).to(dev), n


def run_shape(name, group, dims, n_keys, kind, cold_share=0.0):
    nt, B = len(dims), args.bags
    W = sum(dims)
    keys, off, n = batch_for(nt, n_keys, seed=nt, cold_share=cold_share)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    located = None if kind == "tiered" else torch.empty(n, dtype=torch.int64, device=dev)
    index = torch.zeros(n, dtype=torch.int32, device=dev)
    loc_kw = {} if located is None else {"located": located}
    flat = {dt: torch.empty(B * W, dtype=dt, device=dev) for dt in (torch.float32, BF16)}     # the table-major (class-major) result: one buffer, re-read by the copy
    blocks = {dt: [torch.empty((B, W), dtype=dt, device=dev) for _ in range(ROT)] for dt in (torch.float32, BF16)}

    def table_major(dt):
        if kind == "mixed":
            return group.find_pooled(keys, off, "mean", out=flat[dt], found=found, out_dtype=dt, **loc_kw)[0]
        return group.find_pooled(keys, off, "mean", out=flat[dt].view(nt * B, dims[0]), found=found, out_dtype=dt, **loc_kw)[0]

    def composed_fwd(i, dt):
        r = table_major(dt)
        if kind == "mixed":
            torch.cat(r, dim=1, out=blocks[dt][i % ROT])
        else:
            blocks[dt][i % ROT].view(B, nt, dims[0]).copy_(r.view(nt, B, dims[0]).transpose(0, 1))

    def keyed_fwd(i, dt, with_index=True):
        group.find_pooled(keys, off, "mean", out=blocks[dt][i % ROT], found=found, out_dtype=dt, layout="keyed", step_index=index if with_index else None, **loc_kw)

    rows = {"composed fwd fp32": lambda i: composed_fwd(i, torch.float32), "keyed fwd fp32": lambda i: keyed_fwd(i, torch.float32),
            "table-major fwd fp32": lambda i: table_major(torch.float32), "keyed, no index fwd fp32": lambda i: keyed_fwd(i, torch.float32, False),
            "composed fwd bf16": lambda i: composed_fwd(i, BF16), "keyed fwd bf16": lambda i: keyed_fwd(i, BF16),
            "table-major fwd bf16": lambda i: table_major(BF16)}
    # the two forwards write the same block
    composed_fwd(0, torch.float32)
    keyed_fwd(1, torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(blocks[torch.float32][0].view(torch.int32), blocks[torch.float32][1].view(torch.int32)), "the keyed block is the composition's"

    grad = torch.randn((B, W), device=dev) * 1e-3      # the dense network's gradient of the block

    def composed_bwd(i):
        lens = off[1:] - off[:-1]
        bag_of = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens, output_size=n)
        inv = lens.clamp(min=1).to(torch.float32)
        if kind == "mixed":
            g = torch.empty(B * W, device=dev)
            for j, (v, piece) in enumerate(zip(group.views(g, B), torch.split(grad, list(dims), dim=1))):   # autograd's backward of the cat, then the layer's division per member
                v.copy_(piece)
                v /= inv[j * B:(j + 1) * B, None]
            group.apply_pooled(keys, off, g, bag_of, "adagrad", 1e-3, located=located)
        else:
            g = grad.view(B, nt, dims[0]).transpose(0, 1).reshape(nt * B, dims[0])                         # the permute-back copy
            g = g / inv[:, None]
            group.apply_pooled(keys, off, g, bag_of, "adagrad", 1e-3, **loc_kw)

    def keyed_bwd(i):
        if kind == "mixed":
            group.apply_pooled(keys, off, grad, index, "adagrad", 1e-3, located=located, layout="keyed", mean_offsets=off)
        else:
            inv = (off[1:] - off[:-1]).clamp(min=1).to(torch.float32)
            g = grad.view(B, nt, dims[0]) / inv.view(nt, B).t()[:, :, None]
            group.apply_pooled(keys, off, g.view(B * nt, dims[0]), index, "adagrad", 1e-3, **loc_kw)

    keyed_fwd(0, torch.float32)   # located and index of this batch for the steps
    rows["composed bwd"] = composed_bwd
    rows["keyed bwd"] = keyed_bwd
    us = timed_rows(rows, args.reps)
    rec = {"n": n, "tables": nt, "bags_per_table": B, "width": W, "block_bytes_fp32": B * W * 4, "us": {k: round(v, 2) for k, v in us.items()}}
    results.setdefault(name, []).append(rec)
    print(name, json.dumps(rec), flush=True)


def populate_range(table, start, count, dim, chunk=1 << 20):
    for s in range(start, start + count, chunk):
        k = synth.keys_t(1, s, min(chunk, start + count - s), dev)
        table.insert(k, synth.rows_t(k, dim, 2))
    torch.cuda.synchronize(dev)


def members(dims, n_keys):
    out = []
    for d in dims:
        t = LookupTable(int(n_keys / 0.75), d, device=dev, max_batch=1 << 21, optimizer=OPT_ADAGRAD)
        bench.populate(t, synth, n_keys, d, dev, 1 << 20)
        out.append(t)
    return out


def make_pair(n_keys, dim):
    hot = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=1 << 21, optimizer=OPT_ADAGRAD)
    cold = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=1 << 21, optimizer=OPT_ADAGRAD, value_memory=_lib.MEM_HOST_PINNED)
    populate_range(hot, 0, n_keys, dim)
    populate_range(cold, n_keys, n_keys, dim)
    return TieredLookupTable(hot, cold, hot_key_limit=int(n_keys / 0.75))


def summarize(res):
    summary = {}
    for shape, (a, b) in res.items():
        out = {k: a[k] for k in a if k != "us"}
        for what, base in (("fwd fp32", "composed"), ("fwd bf16", "composed"), ("fwd fp32", "table-major"), ("fwd bf16", "table-major"), ("bwd", "composed"),
                           ("fwd fp32, no index", "table-major")):
            f, s = (f"keyed {what}", f"{base} {what}") if "no index" not in what else ("keyed, no index fwd fp32", "table-major fwd fp32")
            mf, ms = (a["us"][f] + b["us"][f]) / 2, (a["us"][s] + b["us"][s]) / 2
            spread = max(abs(a["us"][f] - b["us"][f]), abs(a["us"][s] - b["us"][s]))
            out[f"{what} vs {base}"] = {"keyed_us": round(mf, 2), f"{base}_us": round(ms, 2), "speedup": round(ms / mf, 3), "spread_us": round(spread, 2),
                                        "verdict": "faster" if mf < ms - spread else "slower" if mf > ms + spread else "level"}
        summary[shape] = out
    return summary


what = args.what.split(",")
cap = 1 << 21
if "uniform" in what:
    ms = members([args.dim] * args.tables, args.group_keys)
    group = TableGroup(ms, max_apply_batch=cap)
    for p in range(2):
        run_shape(f"uniform {args.tables} x dim {args.dim}", group, [args.dim] * args.tables, args.group_keys, "uniform")
    group.close()
    for m in ms:
        m.close()
    torch.cuda.empty_cache()
if "tiered" in what:
    pairs = [make_pair(args.group_keys, args.dim) for _ in range(args.tables)]
    tgroup = TieredTableGroup(pairs, max_apply_batch=cap)
    for p in range(2):
        run_shape(f"pairs {args.tables} x dim {args.dim}, a tenth cold", tgroup, [args.dim] * args.tables, args.group_keys, "tiered", cold_share=0.1)
    tgroup.close()
    for pr in pairs:
        pr.hot.close(); pr.cold.close()
    torch.cuda.empty_cache()
if "mixed" in what:
    ms = members(MIXED_DIMS, args.group_keys)
    mgroup = MixedTableGroup(ms, max_apply_batch=cap)
    for p in range(2):
        run_shape(f"mixed {MIXED_DIMS}", mgroup, MIXED_DIMS, args.group_keys, "mixed")
    mgroup.close()
    for m in ms:
        m.close()
print("KEYED_POOLED_BENCH " + json.dumps(summarize(results)), flush=True)
