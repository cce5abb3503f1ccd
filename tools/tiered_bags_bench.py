"""Embedding bags over the hot/cold pair (TieredLookupTable.find_pooled, mee_find_pooled_tiered): dim 64, 256K keys per call in bags of 8 and of 20.
 (a) the pair whose hot tier holds the whole working set against ONE table holding the same keys (mee_find_pooled);
 (b) at cold shares 0 / 5 / 20 % of the positions: the pair's find_pooled against the route without it — TieredLookupTable.find ([n, dim] fp32 rows,
     two launches) + a torch sum over each bag's rows (the bags have one length here, so the cheapest torch form: rows.view(bags, L, dim).sum(1));
 (c) one DynamicEmbeddingBag training step (forward + backward with the sparse Adagrad step) over the pair.
The sides of a comparison alternate inside one process, round by round; per side: median and min over the rounds and the spread (max - min) / median.
usage: python tools/tiered_bags_bench.py [--hot KEYS] [--cold KEYS] [--rounds R] [--reps N]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from meepoembedding_amd import OPT_ADAGRAD, LookupTable, _lib, synth
from meepoembedding_amd.nn import DynamicEmbeddingBag
from meepoembedding_amd.tiered import TieredLookupTable

ap = argparse.ArgumentParser()
ap.add_argument("--hot", type=int, default=4_000_000)
ap.add_argument("--cold", type=int, default=1_000_000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=60)
args = ap.parse_args()
dev = torch.device("cuda", 0)
dim, B, chunk = 64, 1 << 18, 1 << 20
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def fill(table, start, count):
    for s in range(start, start + count, chunk):
        k = synth.keys_t(1, s, min(chunk, start + count - s), dev)
        table.insert(k, synth.rows_t(k, dim, 2))
    torch.cuda.synchronize(dev)


def batches(cold_share, n, seed, n_batches=8):
    """positions drawn uniformly from the hot keys, a cold_share of them (at random positions) from the cold keys"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = []
    for _ in range(n_batches):
        idx = torch.randint(0, args.hot, (n,), device=dev, generator=g)
        if cold_share:
            cold = torch.rand(n, device=dev, generator=g) < cold_share
            idx = torch.where(cold, args.hot + torch.randint(0, args.cold, (n,), device=dev, generator=g), idx)
        out.append(synth.mix64_t((idx + 1) * synth._s64(synth._GOLDEN) + synth._s64(1)))
    return out


def events(fn, reps):
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / reps


def compare(sides, reps):
    """sides: {name: fn(i)} -> {name: (median us, min us, spread)}; warm-up, then the sides alternate round by round"""
    for fn in sides.values():
        for i in range(10):
            fn(i)
    torch.cuda.synchronize(dev)
    t = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            t[name].append(events(fn, reps))
    return {name: (statistics.median(v), min(v), (max(v) - min(v)) / statistics.median(v)) for name, v in t.items()}


def show(res):
    return "; ".join(f"{name} median {m:.1f} us, min {lo:.1f} us, spread {s * 100:.1f} %" for name, (m, lo, s) in res.items())


print(f"dim {dim}, {B} keys per call; hot tier {args.hot} keys in HBM, cold tier {args.cold} keys with rows in pinned host memory; one table of the "
      f"union beside them; {args.rounds} rounds x {args.reps} calls per side, sides alternating", flush=True)
hot = LookupTable(int(args.hot / 0.75), dim, device=dev, max_batch=chunk)
cold = LookupTable(int(args.cold / 0.75), dim, device=dev, max_batch=chunk, value_memory=_lib.MEM_HOST_PINNED)
one = LookupTable(int((args.hot + args.cold) / 0.75), dim, device=dev, max_batch=chunk)
fill(hot, 0, args.hot); fill(cold, args.hot, args.cold); fill(one, 0, args.hot + args.cold)
pair = TieredLookupTable(hot, cold, hot_key_limit=args.hot)

for L in (8, 20):
    nb = B // L
    n = nb * L
    off = torch.arange(nb + 1, dtype=torch.int64, device=dev) * L
    out_p, out_o = torch.empty((nb, dim), device=dev), torch.empty((nb, dim), device=dev)
    f_p, f_o = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    for share in (0.0, 0.05, 0.20):
        ks = batches(share, n, seed=int(share * 100) + L)
        a, _ = pair.find_pooled(ks[0], off, "sum")
        b, _ = one.find_pooled(ks[0], off, "sum")
        assert torch.equal(a, b), "the pair must pool like one table of the union"
        sides = {"pair.find_pooled": lambda i: pair.find_pooled(ks[i % 8], off, "sum", out=out_p, found=f_p)}
        if share == 0.0:
            sides["one-table find_pooled"] = lambda i: one.find_pooled(ks[i % 8], off, "sum", out=out_o, found=f_o)
        sides["pair.find + torch bag sum"] = lambda i: pair.find(ks[i % 8])[0].view(nb, L, dim).sum(1)
        print(f"bags of {L} ({nb} bags), cold share {share * 100:.0f} %: {show(compare(sides, args.reps))}", flush=True)

# (c) one training step of the bag layer over the pair: forward (find_pooled) + backward (the indexed sparse Adagrad step on both tiers)
del one
torch.cuda.empty_cache()
hot_t = LookupTable(int(args.hot / 0.75), dim, device=dev, max_batch=chunk, optimizer=OPT_ADAGRAD, initial_accumulator=0.1)
cold_t = LookupTable(int(args.cold / 0.75), dim, device=dev, max_batch=chunk, optimizer=OPT_ADAGRAD, initial_accumulator=0.1, value_memory=_lib.MEM_HOST_PINNED)
fill(hot_t, 0, args.hot); fill(cold_t, args.hot, args.cold)
layer = DynamicEmbeddingBag(TieredLookupTable(hot_t, cold_t, hot_key_limit=args.hot), mode="sum", optimizer="adagrad", lr=0.01).to(dev).train()
for L in (8, 20):
    nb = B // L
    off = torch.arange(nb + 1, dtype=torch.int64, device=dev) * L
    head = torch.randn(nb, dim, device=dev) * 0.01
    for share in (0.0, 0.05):
        ks = batches(share, nb * L, seed=50 + int(share * 100) + L)

        def step(i):
            (layer(ks[i % 8], off) * head).sum().backward()

        for i in range(5):
            step(i)
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for i in range(20):
                step(i)
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e6 / 20)
        print(f"training step, bags of {L}, cold share {share * 100:.0f} %: median {statistics.median(ts):.1f} us, min {min(ts):.1f} us, "
              f"spread {(max(ts) - min(ts)) / statistics.median(ts) * 100:.1f} % (host clock around 20 steps ending in a synchronise)", flush=True)
