"""The padded sequence lookup (SPEC.md §3 "find_padded") against what a user without it runs for the same [n_bags, max_len, dim] block.

Forward, baseline: find into [n, dim], a zeroed [n_bags * L + 1, dim] block, ONE indexed placement (index_copy_ with a precomputed slot per position;
cut-off positions go to a spare row) — the index arithmetic is not timed.  Forward, fused: find_padded.
Backward (fp32, Adagrad), baseline: the gather of the dense grad back to [n, dim], then apply_adagrad with the cut-off keys blanked.  Fused:
apply_adagrad(step_keys, dense grad, grad_index=...) — for a group apply_indexed.
Per shape the rows take turns inside ONE timing loop, in chunks of 10 calls between device events of their own, result buffers rotating; the
whole sequence runs twice and the spread of a comparison is the largest pass-to-pass difference of the two rows compared.
Bytes (algorithmic): fused forward = kept * (8 + 128 + row) + n_bags * L * dim * out_elem; the baseline adds 2 * n * dim * 4 (the [n, dim] array
written and read back) and the block's zero fill.
usage: python tools/find_padded_bench.py [--keys N] [--group-keys N] [--reps K] [--bags B] [--tables T]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from meepoembedding_amd import OPT_ADAGRAD, LookupTable, TableGroup, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=10_000_000, help="keys in the single table")
ap.add_argument("--group-keys", type=int, default=1_000_000, help="keys in every member of the group")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--bags", type=int, default=2048, help="bags per table")
ap.add_argument("--tables", type=int, default=26)
ap.add_argument("--dims", default="64,128")
args = ap.parse_args()
dev = torch.device("cuda", 0)
BF16, ROT, EMPTY = torch.bfloat16, 4, -(1 << 63)
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


def batch_for(n_tables, n_keys, mean, L, seed):
    """bag lengths geometric with the given mean (a tail past L), keys uniform over each member's stored keys"""
    rng = np.random.default_rng(seed)
    lens = rng.geometric(1.0 / (mean + 1), n_tables * args.bags) - 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    keys = synth.keys_t(1, 0, n_keys, dev)[torch.randint(0, n_keys, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(seed))]
    begin = np.repeat(off[:-1], lens)
    j = np.arange(n) - begin                       # keep="first": position begin + j fills slot j
    slot = np.where(j < L, np.repeat(np.arange(lens.size), lens) * L + j, lens.size * L)   # cut-off positions: the spare row
    return keys.contiguous(), torch.from_numpy(off).to(dev), torch.from_numpy(slot).to(dev), int(np.minimum(lens, L).sum()), n, float((lens > L).mean())


def run_shape(name, table, group, dim, n_keys, mean, L):
    n_tables = len(group.tables) if group is not None else 1
    keys, off, slot, kept, n, tail = batch_for(n_tables, n_keys, mean, L, seed=mean)
    n_bags = n_tables * args.bags
    seg = off[::args.bags].contiguous()
    rows_n = torch.empty((n, dim), device=dev)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    blocks = {torch.float32: [torch.empty((n_bags * L + 1, dim), device=dev) for _ in range(ROT)],
              BF16: [torch.empty((n_bags * L + 1, dim), dtype=BF16, device=dev) for _ in range(ROT)]}
    rows_16 = torch.empty((n, dim), dtype=BF16, device=dev)
    target = group if group is not None else table

    def base_fwd(i, dt):
        if group is not None:
            group.find(keys, seg, out=rows_n if dt == torch.float32 else rows_16, found=found, out_dtype=dt)
        else:
            table.find(keys, out=rows_n if dt == torch.float32 else rows_16, found=found, out_dtype=dt)
        b = blocks[dt][i % ROT]
        b.zero_()
        b.index_copy_(0, slot, rows_n if dt == torch.float32 else rows_16)

    def fused_fwd(i, dt):
        target.find_padded(keys, off, L, out=blocks[dt][i % ROT][:n_bags * L], found=found, out_dtype=dt)

    rows = {"baseline fwd fp32": lambda i: base_fwd(i, torch.float32), "fused fwd fp32": lambda i: fused_fwd(i, torch.float32),
            "baseline fwd bf16": lambda i: base_fwd(i, BF16), "fused fwd bf16": lambda i: fused_fwd(i, BF16)}
    # backward: the dense grad of the block, fp32
    grad = torch.randn((n_bags * L + 1, dim), device=dev) * 1e-3
    grad[-1].zero_()
    _, _, _, step_keys, grad_index = target.find_padded(keys, off, L, with_step=True)
    blanked = torch.where(slot < n_bags * L, keys, torch.full_like(keys, EMPTY))
    assert torch.equal(blanked, step_keys)

    def base_bwd(i):
        g = grad.index_select(0, slot)
        if group is not None:
            group.apply_adagrad(blanked, seg, g, 1e-3)
        else:
            table.apply_adagrad(blanked, g, 1e-3)

    def fused_bwd(i):
        if group is not None:
            group.apply_indexed(step_keys, seg, grad[:n_bags * L], grad_index, "adagrad", 1e-3)
        else:
            table.apply_adagrad(step_keys, grad[:n_bags * L], 1e-3, grad_index=grad_index)

    rows["baseline bwd"] = base_bwd
    rows["fused bwd"] = fused_bwd
    us = timed_rows(rows, args.reps)
    rec = {"n": n, "kept": kept, "share_of_bags_past_L": round(tail, 3), "us": {k: round(v, 2) for k, v in us.items()}}
    for dt, eb in (("fp32", 4), ("bf16", 2)):
        fused_b = kept * (8 + 128 + 4 * dim) + n_bags * L * dim * eb
        base_b = n * (8 + 128 + 4 * dim) + 2 * n * dim * eb + 2 * n_bags * L * dim * eb
        rec[f"bytes fwd {dt}"] = {"fused": fused_b, "baseline": base_b, "fused_TBps": round(fused_b / us[f"fused fwd {dt}"] / 1e6, 3),
                                  "write_bound_us_at_4TBps": round(n_bags * L * dim * eb / 4e6, 2)}
    results.setdefault(name, []).append(rec)
    print(name, json.dumps(rec), flush=True)


for dim in [int(d) for d in args.dims.split(",")]:
    table = LookupTable(int(args.keys / 0.75), dim, device=dev, max_batch=1 << 20, optimizer=OPT_ADAGRAD)
    bench.populate(table, synth, args.keys, dim, dev, 1 << 20)
    members = [LookupTable(int(args.group_keys / 0.75), dim, device=dev, max_batch=1 << 21, optimizer=OPT_ADAGRAD) for _ in range(args.tables)]
    for m in members:
        bench.populate(m, synth, args.group_keys, dim, dev, 1 << 20)
    group = TableGroup(members, max_apply_batch=1 << 21)
    print(f"dim {dim}: one table of {args.keys} keys ({table.table_bytes / 1e9:.2f} GB), a group of {args.tables} x {args.group_keys} keys; {args.bags} bags per table; "
          f"{ROT} rotating blocks; {args.reps} timed calls per row and pass", flush=True)
    for p in range(2):
        for mean, L in ((8, 20), (20, 50)):
            run_shape(f"table dim {dim} mean {mean} L {L}", table, None, dim, args.keys, mean, L)
            run_shape(f"group dim {dim} mean {mean} L {L}", None, group, dim, args.group_keys, mean, L)
    group.close()
    for m in members + [table]:
        m.close()
    torch.cuda.empty_cache()

summary = {}
for shape, (a, b) in results.items():
    out = {"n": a["n"], "kept": a["kept"], "bytes fwd fp32": a["bytes fwd fp32"], "bytes fwd bf16": a["bytes fwd bf16"]}
    for what in ("fwd fp32", "fwd bf16", "bwd"):
        f, s = f"fused {what}", f"baseline {what}"
        mf, ms = (a["us"][f] + b["us"][f]) / 2, (a["us"][s] + b["us"][s]) / 2
        spread = max(abs(a["us"][f] - b["us"][f]), abs(a["us"][s] - b["us"][s]))
        out[what] = {"fused_us": round(mf, 2), "baseline_us": round(ms, 2), "speedup": round(ms / mf, 3), "spread_us": round(spread, 2),
                     "verdict": "faster" if mf < ms - spread else "slower" if mf > ms + spread else "level"}
    summary[shape] = out
print("FIND_PADDED_BENCH " + json.dumps(summary), flush=True)
