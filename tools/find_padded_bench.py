"""The padded sequence lookup (SPEC.md §3 "find_padded") against what a user without it runs for the same [n_bags, max_len, dim] block.

Forward, baseline: find into [n, dim], a zeroed [n_bags * L + 1, dim] block, ONE indexed placement (index_copy_ with a precomputed slot per position;
cut-off positions go to a spare row) — the index arithmetic is not timed.  Forward, fused: find_padded.
Backward (fp32, Adagrad), baseline: the gather of the dense grad back to [n, dim], then apply_adagrad with the cut-off keys blanked.  Fused:
apply_adagrad(step_keys, dense grad, grad_index=...) — for a group apply_indexed.
Per shape the rows take turns inside ONE timing loop, in chunks of 10 calls between device events of their own, result buffers rotating; the
whole sequence runs twice and the spread of a comparison is the largest pass-to-pass difference of the two rows compared.
Bytes (algorithmic): fused forward = kept * (8 + 128 + row) + n_bags * L * dim * out_elem; the baseline adds 2 * n * dim * 4 (the [n, dim] array
written and read back) and the block's zero fill.
--what tiered: the same comparison over a hot/cold pair and a group of pairs (the cold rows in pinned host memory), every lookup hot and a tenth of
them cold; the baseline there is the composition nn.lookup_padded ran before the tiered forms existed (run_tiered_shape).
usage: python tools/find_padded_bench.py [--what plain|tiered|all] [--keys N] [--group-keys N] [--pair-keys N] [--pair-group-keys N] [--reps K]
       [--bags B] [--tables T]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from meepoembedding_amd import OPT_ADAGRAD, LookupTable, TableGroup, _lib, synth
from meepoembedding_amd.tiered import TieredLookupTable, TieredTableGroup

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=10_000_000, help="keys in the single table")
ap.add_argument("--group-keys", type=int, default=1_000_000, help="keys in every member of the group")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--bags", type=int, default=2048, help="bags per table")
ap.add_argument("--tables", type=int, default=26)
ap.add_argument("--dims", default="64,128")
ap.add_argument("--what", default="plain", choices=["plain", "tiered", "all"], help="plain: one table and a group; tiered: a hot/cold pair and a group of pairs")
ap.add_argument("--pair-keys", type=int, default=10_000_000, help="keys in each tier of the single pair")
ap.add_argument("--pair-group-keys", type=int, default=1_000_000, help="keys in each tier of every pair of the group of pairs")
args = ap.parse_args()
dev = torch.device("cuda", 0)
BF16, ROT, EMPTY = torch.bfloat16, 4, -(1 << 63)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
results, tiered_results = {}, {}


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


def populate_range(table, start, count, dim, chunk=1 << 20):
    for s in range(start, start + count, chunk):
        k = synth.keys_t(1, s, min(chunk, start + count - s), dev)
        table.insert(k, synth.rows_t(k, dim, 2))
    torch.cuda.synchronize(dev)


def make_pair(n_keys, dim, max_batch):
    """a hot/cold pair: keys 0 .. n_keys in the hot table (HBM), n_keys .. 2 n_keys in the cold one (rows and state in pinned host memory)"""
    hot = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=max_batch, optimizer=OPT_ADAGRAD)
    cold = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=max_batch, optimizer=OPT_ADAGRAD, value_memory=_lib.MEM_HOST_PINNED)
    populate_range(hot, 0, n_keys, dim)
    populate_range(cold, n_keys, n_keys, dim)
    return TieredLookupTable(hot, cold, hot_key_limit=int(n_keys / 0.75))


def run_tiered_shape(name, pair, tgroup, dim, n_keys, mean, L, cold_share):
    """The tiered forms against the composition nn.lookup_padded runs without them (the parent commit's path over a pair or a TieredTableGroup): find of
    the kept keys into [n_kept, dim] — the pair's two launches, the group's mee_group_find_tiered — a zero fill of the block and a scatter; backward:
    the gather of the kept slots' grad rows, then the plain step.  The index arithmetic and the gather of the kept keys are not timed.
    The pair's find takes no out=: its [n_kept, dim] result comes from torch's caching allocator on every call, as it does in the layer's composition
    (the group's find writes into a buffer kept here); the fused rows allocate nothing.
    cold_share: the share of the positions whose key sits in the cold tier."""
    n_tables = len(tgroup.tables) if tgroup is not None else 1
    keys, off, slot, kept, n, tail = batch_for(n_tables, n_keys, mean, L, seed=mean)
    if cold_share:
        gen = torch.Generator(device=dev).manual_seed(mean + 1)
        cold_keys = synth.keys_t(1, n_keys, n_keys, dev)[torch.randint(0, n_keys, (n,), device=dev, generator=gen)]
        keys = torch.where(torch.rand(n, device=dev, generator=gen) < cold_share, cold_keys, keys).contiguous()
    n_bags = n_tables * args.bags
    seg = off[::args.bags].contiguous()
    target = tgroup if tgroup is not None else pair
    pos = torch.nonzero(slot < n_bags * L).view(-1)
    kk, kslot = keys[pos].contiguous(), slot[pos].contiguous()
    seg_kept = torch.searchsorted(pos, seg).contiguous()
    rows_k = torch.empty((kept, dim), device=dev)
    found_k = torch.empty(kept, dtype=torch.uint8, device=dev)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    blocks = [torch.empty((n_bags * L, dim), device=dev) for _ in range(ROT)]

    def base_fwd(i):
        rows = tgroup.find(kk, seg_kept, out=rows_k, found=found_k)[0] if tgroup is not None else pair.find(kk)[0]
        b = blocks[i % ROT]
        b.zero_()
        b.index_copy_(0, kslot, rows)

    def fused_fwd(i):
        target.find_padded(keys, off, L, out=blocks[i % ROT], found=found)

    grad = torch.randn((n_bags * L, dim), device=dev) * 1e-3
    fo, _, _, step_keys, grad_index = target.find_padded(keys, off, L, with_step=True)
    base_fwd(0)
    assert torch.equal(fo.view(-1, dim), blocks[0]), "the fused block is the composition's"

    def base_bwd(i):
        g = grad.index_select(0, kslot)
        if tgroup is not None:
            tgroup.apply_adagrad(kk, seg_kept, g, 1e-3)
        else:
            pair.apply_adagrad(kk, g, 1e-3)

    def fused_bwd(i):
        if tgroup is not None:
            tgroup.apply_indexed(step_keys, seg, grad, grad_index, "adagrad", 1e-3)
        else:
            pair.apply_adagrad(step_keys, grad, 1e-3, grad_index=grad_index)

    us = timed_rows({"baseline fwd fp32": base_fwd, "fused fwd fp32": fused_fwd, "baseline bwd": base_bwd, "fused bwd": fused_bwd}, args.reps)
    rec = {"n": n, "kept": kept, "cold_share": cold_share, "us": {k: round(v, 2) for k, v in us.items()}}
    tiered_results.setdefault(name, []).append(rec)
    print(name, json.dumps(rec), flush=True)


def tiered_shapes(dim):
    pair = make_pair(args.pair_keys, dim, 1 << 20)
    pairs = [make_pair(args.pair_group_keys, dim, 1 << 21) for _ in range(args.tables)]
    tgroup = TieredTableGroup(pairs, max_apply_batch=1 << 21)
    print(f"dim {dim}: one pair of {args.pair_keys} + {args.pair_keys} keys, {args.tables} pairs of {args.pair_group_keys} + {args.pair_group_keys}; cold rows in pinned host memory", flush=True)
    for p in range(2):
        for mean, L in ((8, 20), (20, 50)):
            for share in (0.0, 0.1):
                what = "all hot" if not share else "a tenth cold"
                run_tiered_shape(f"pair dim {dim} mean {mean} L {L} {what}", pair, None, dim, args.pair_keys, mean, L, share)
                run_tiered_shape(f"pairs dim {dim} mean {mean} L {L} {what}", None, tgroup, dim, args.pair_group_keys, mean, L, share)
    tgroup.close()
    for pr in pairs + [pair]:
        pr.hot.close(); pr.cold.close()
    torch.cuda.empty_cache()


def summarize(res, whats):
    summary = {}
    for shape, (a, b) in res.items():
        out = {k: a[k] for k in a if k != "us"}
        for what in whats:
            f, s = f"fused {what}", f"baseline {what}"
            mf, ms = (a["us"][f] + b["us"][f]) / 2, (a["us"][s] + b["us"][s]) / 2
            spread = max(abs(a["us"][f] - b["us"][f]), abs(a["us"][s] - b["us"][s]))
            out[what] = {"fused_us": round(mf, 2), "baseline_us": round(ms, 2), "speedup": round(ms / mf, 3), "spread_us": round(spread, 2),
                         "verdict": "faster" if mf < ms - spread else "slower" if mf > ms + spread else "level"}
        summary[shape] = out
    return summary


for dim in [int(d) for d in args.dims.split(",")]:
    if args.what in ("tiered", "all"):
        tiered_shapes(dim)
    if args.what == "tiered":
        continue
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

if results:
    print("FIND_PADDED_BENCH " + json.dumps(summarize(results, ("fwd fp32", "fwd bf16", "bwd"))), flush=True)
if tiered_results:
    print("FIND_PADDED_TIERED_BENCH " + json.dumps(summarize(tiered_results, ("fwd fp32", "bwd"))), flush=True)
