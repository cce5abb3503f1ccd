"""GPU tuning harness for the find kernel: interleaved variants in ONE process, median/min launch time per variant.
usage: python tools/tune_find.py [--keys 100000000] [--batch 262144] [--rounds 5] knob=value,knob=value ...
--batches 65536,131072,262144,524288,1048576: a launch-size sweep over ONE populated table, with the least-squares fit
time = floor + slope * (keys / 256K) per variant behind it (the floor is what a launch costs whatever its size)."""
import argparse, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from meepoembedding_amd import LookupTable, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=100_000_000)
ap.add_argument("--batch", type=int, default=1 << 18)
ap.add_argument("--batches", default=None, help="comma-separated launch sizes: sweep them in this process and fit floor + slope per variant")
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--dist", default="uniform")
ap.add_argument("--no-found", action="store_true")
ap.add_argument("--miss", type=float, default=0.0, help="fraction of looked-up keys that are absent")
ap.add_argument("--load", type=float, default=0.75)
ap.add_argument("--out-buffers", type=int, default=1, help="result buffers used in turn (6 x 64 MB: nothing of a launch's output is still cached when its buffer comes round again)")
ap.add_argument("variants", nargs="*", default=["find_rounds=1", "find_rounds=2", "find_rounds=4", "find_rounds=8"])
a = ap.parse_args()
dev = torch.device("cuda", 0)
t = LookupTable(int(a.keys / a.load), a.dim, device=dev, max_batch=1 << 20)
bench.populate(t, synth, a.keys, a.dim, dev, 1 << 20)
sizes = [int(x) for x in a.batches.split(",")] if a.batches else [a.batch]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
defaults = {"find_rounds": 2, "find_grid_cap": 0, "find_nt": -1, "find_block": 256}
bpl = bench.algorithmic_bytes_per_lookup(a.dim)
medians = {v: [] for v in a.variants}
for batch in sizes:
    batches = bench.lookup_batches(synth, a.keys, batch, 64, a.dist, dev, seed=3)
    if a.miss > 0:
        g_ = torch.Generator(device=dev); g_.manual_seed(5)
        for b in batches:
            m = torch.rand(batch, device=dev, generator=g_) < a.miss
            b[m] = synth.keys_t(99, 0, batch, dev)[m]   # keys of another stream: absent
    outs = [torch.empty((batch, a.dim), dtype=torch.float32, device=dev) for _ in range(a.out_buffers)]; found = None if a.no_found else torch.empty(batch, dtype=torch.uint8, device=dev)
    times = {v: [] for v in a.variants}
    for r in range(a.rounds + 1):
        for v in a.variants:
            for k, d in defaults.items():
                t.set_tuning(k, d)
            for kv in v.split(","):
                k, val = kv.split("="); t.set_tuning(k, int(val))
            for i in range(10):
                t.find(batches[i % 64], out=outs[i % a.out_buffers], found=found, want_found=not a.no_found)
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.launches):
                t.find(batches[i % 64], out=outs[i % a.out_buffers], found=found, want_found=not a.no_found)
            e1.record(); torch.cuda.synchronize()
            if r:
                times[v].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    for v, ts in times.items():
        med, mn = statistics.median(ts), min(ts)
        medians[v].append(med)
        print(f"{(str(batch) + ' ' if a.batches else '') + v:40s} median {med:7.2f} us  min {mn:7.2f} us  -> {batch / med / 1e3:6.2f} Gkeys/s  {batch * bpl / med / 1e3:7.1f} GB/s  frac {batch * bpl / med / 1e3 / 8000:.3f}")
    del batches, outs
if len(sizes) > 1:
    xs = [s / 262144 for s in sizes]
    for v, ys in medians.items():
        mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
        slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
        print(f"fit {v:36s} floor {my - slope * mx:6.2f} us  slope {slope:6.2f} us per 256K keys")
