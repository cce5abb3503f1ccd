"""The FTRL-Proximal step against the Adam and Adagrad steps of the same tree (profiles/ftrl.md): the configs[2] shape — dim 64, 256K-key batches,
uniform and Zipf(1.05) ids over one table per optimizer with the same keys — as a located training forward plus the step on its handles, and the
grouped 26-table dim-64 bag step (2048 bags per table).

The optimizers take turns in chunks of 10 calls inside ONE timing loop, each chunk between device events of its own; the whole sequence runs
twice, and the spread of a comparison is the largest pass-to-pass difference of the rows compared.  FTRL's yardstick is Adam: both move the
same bytes per step (264 B per position + 1544 B per distinct key: the row and two state planes read and written) through the same kernel body.
No bar is set: the ratio and the spread are reported, and whether FTRL is slower beyond the spread.
usage: python tools/ftrl_bench.py [--keys N] [--reps K] [--skip-group]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, OPT_FTRL, LookupTable, TableGroup, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=100_000_000, help="keys per table (three tables live at once: 100M keys need about 280 GB)")
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--skip-group", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
DIM, BATCH = 64, 1 << 18
KINDS = (("adagrad", OPT_ADAGRAD), ("adam", OPT_ADAM), ("ftrl", OPT_FTRL))
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
    return {nm: round(total[nm] / (reps // chunk * chunk), 2) for nm in names}


def step_of(t, kind, keys, grads, slots, i):
    """one optimizer step on the handles of this step's forward; Adam's step number moves"""
    if kind == "adagrad":
        t.apply_adagrad(keys, grads, lr=0.01, slots=slots)
    elif kind == "adam":
        t.apply_adam(keys, grads, lr=0.001, step=i + 1, slots=slots)
    else:
        t.apply_ftrl(keys, grads, lr=0.05, beta=1.0, l1=0.001, l2=0.001, slots=slots)


def table_rows(tabs, dist):
    batches = bench.lookup_batches(synth, args.keys, BATCH, 8, dist, dev, seed=3)
    grads = [torch.randn(BATCH, DIM, device=dev) * 0.01 for _ in range(2)]
    out = torch.empty((BATCH, DIM), device=dev)
    found, slots = torch.empty(BATCH, dtype=torch.uint8, device=dev), torch.empty(BATCH, dtype=torch.int64, device=dev)
    rows = {}
    for kind, _ in KINDS:
        def run(i, t=tabs[kind], kind=kind):
            k = batches[i % 8]
            t.find_located(k, out=out, found=found, slots=slots, prepare_apply=True)
            step_of(t, kind, k, grads[i % 2], slots, i)
        rows[kind] = run
    us = timed_rows(rows, args.reps)
    shape = f"located forward + step, dim {DIM}, batch {BATCH}, {dist}"
    results.setdefault(shape, []).append(us)
    print(shape, json.dumps(us), flush=True)


def group_rows(groups, keys, off, bag_of, n_bags):
    grads = torch.randn(n_bags, DIM, device=dev) * 0.01
    rows = {}
    for kind in ("adam", "ftrl"):
        g = groups[kind]
        located = torch.empty(keys.numel(), dtype=torch.int64, device=dev)

        def run(i, g=g, kind=kind, located=located):
            g.find_pooled(keys, off, "sum", located=located)
            if kind == "adam":
                g.apply_pooled(keys, off, grads, bag_of, "adam", 0.001, step=i + 1, located=located)
            else:
                g.apply_pooled(keys, off, grads, bag_of, "ftrl", 0.05, l1=0.001, l2=0.001, located=located)
        rows[kind] = run
    us = timed_rows(rows, args.reps)
    shape = f"26 tables x 2048 bags, dim {DIM}: pooled lookup + grouped step"
    results.setdefault(shape, []).append(us)
    print(shape, json.dumps(us), flush=True)


tabs = {}
for kind, opt in KINDS:
    tabs[kind] = LookupTable(int(args.keys / 0.75), DIM, device=dev, optimizer=opt, max_batch=1 << 20, initial_accumulator=0.1)
    bench.populate(tabs[kind], synth, args.keys, DIM, dev, 1 << 20)
    print(f"{kind}: {args.keys} keys dim {DIM} load 0.75: table_bytes {tabs[kind].table_bytes / 1e9:.2f} GB", flush=True)
groups = None
if not args.skip_group:
    nt, bpt, per_table = 26, 2048, 1_000_000
    gen = torch.Generator(device=dev); gen.manual_seed(5)
    lens = torch.randint(1, 9, (nt * bpt,), device=dev, generator=gen)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    n = int(off[-1].item())
    idx = torch.randint(0, per_table, (n,), device=dev, generator=gen)
    gkeys = synth.mix64_t((idx + 1) * synth._s64(synth._GOLDEN) + synth._s64(1))   # (the ids bench.populate stores)
    bag_of = torch.repeat_interleave(torch.arange(nt * bpt, device=dev), lens, output_size=n)
    groups = {}
    for kind, opt in KINDS[1:]:
        members = [LookupTable(int(per_table / 0.75), DIM, device=dev, optimizer=opt, max_batch=1 << 18, initial_accumulator=0.1) for _ in range(nt)]
        for m in members:
            bench.populate(m, synth, per_table, DIM, dev, 1 << 18)
        groups[kind] = TableGroup(members, max_apply_batch=n)
    print(f"group: {nt} tables x {per_table} keys, {bpt} bags per table, {n} positions", flush=True)
print(f"{args.reps} timed calls per row and pass", flush=True)
for p in range(2):
    print(f"--- pass {p + 1}", flush=True)
    for dist in ("uniform", "zipf"):
        table_rows(tabs, dist)
    if groups:
        group_rows(groups, gkeys, off, bag_of, nt * bpt)
summary = {}
for shape, (a, b) in results.items():
    mean = {k: (a[k] + b[k]) / 2 for k in a}
    spread = max(abs(a["ftrl"] - b["ftrl"]), abs(a["adam"] - b["adam"]))
    summary[shape] = {"pass1": a, "pass2": b, "ftrl_us": round(mean["ftrl"], 2), "adam_us": round(mean["adam"], 2), "ftrl_over_adam": round(mean["ftrl"] / mean["adam"], 4),
                      "spread_us": round(spread, 2), "slower_beyond_spread": mean["ftrl"] > mean["adam"] + spread, "faster_beyond_spread": mean["ftrl"] < mean["adam"] - spread}
print("FTRL_BENCH " + json.dumps(summary), flush=True)
