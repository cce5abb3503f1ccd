"""Eviction by the hit counters: the native operator (mee_evict) against the Python sequence it replaces — mee_hits_scan (synchronises), mee_remove in
chunks of max_batch each followed by .item() (synchronises again), a second scan that resets the counters: LookupTable.evict as it was before the
operator existed, spelled out below with the same kernels — on the same tree and in the same process, the forms taking turns.

One table: dim 64, Adagrad, --keys keys at load 0.75, rows in HBM or (--memory host) in pinned host memory.  The victims are a fixed random set V of 1K,
64K or 1M keys: every key's counter is 1 + (key index mod 3), V's are 0.  The threshold forms run evict(max_hits=0, limit=|V|, reset=True), the
least forms evict(0xFFFFFFFF, |V|, reset=True, least=True): every form evicts exactly V.  After every timed call V is inserted again with its rows
and accumulators and all counters are placed again (not timed), so every call meets the same table.
A call is timed by device events around the whole Python call, the read-back of the count included; reported: the median and min .. max of --reps
calls, and the bytes of the key and counter planes (12 x capacity, what one pass over them reads) over the median.

usage: python tools/evict_bench.py [--keys 10000000] [--reps 9] [--memory hbm|host] [--victims 1024,65536,1048576]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--memory", choices=["hbm", "host"], default="hbm")
ap.add_argument("--victims", type=str, default="1024,65536,1048576")
args = ap.parse_args()
DIM = 64


def sequence_evict(t, max_hits, limit, reset):
    """LookupTable.evict before mee_evict: scan, remove in chunks with a read-back each, reset scan"""
    victims = t.hits_scan(0, max_hits, limit, reset=False)
    removed = 0
    for s in range(0, victims.numel(), t.max_batch):
        removed += int(t.remove(victims[s:s + t.max_batch]).sum().item())
    if reset:
        t.hits_scan(1, 0, 0, reset=True)
    return removed


def main():
    import torch

    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, _lib, synth
    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3, r

    mb = 1 << 20
    t = LookupTable(int(args.keys / 0.75), DIM, device=dev, optimizer=OPT_ADAGRAD, max_batch=mb, track_hits=True, initial_accumulator=0.1,
                    value_memory=_lib.MEM_HBM if args.memory == "hbm" else _lib.MEM_HOST_PINNED)
    keys = synth.keys_t(1, 0, args.keys, dev)
    for s in range(0, args.keys, mb):
        t.insert(keys[s:s + mb], synth.rows_t(keys[s:s + mb], DIM, 2))
    base_hits = (1 + torch.arange(args.keys, device=dev, dtype=torch.int32) % 3)
    scan_bytes = 12 * t.capacity
    results = {}
    forms = {
        "sequence (scan, remove + read-back per chunk, reset scan)": lambda n: sequence_evict(t, 0, n, True),
        "native threshold": lambda n: t.evict(0, n, True),
        "native threshold, spill": lambda n: t.evict(0, n, True, spill=True)[0].numel(),
        "native least": lambda n: t.evict(0xFFFFFFFF, n, True, least=True),
        "native least, spill": lambda n: t.evict(0xFFFFFFFF, n, True, least=True, spill=True)[0].numel(),
    }
    for n in [int(x) for x in args.victims.split(",")]:
        if n > min(mb, args.keys):
            continue
        idx = torch.randperm(args.keys, device=dev)[:n]
        v = keys[idx].contiguous()
        rows, acc = synth.rows_t(v, DIM, 2), synth.rows_t(v, DIM, 3).abs() + 0.1
        hits = base_hits.clone()
        hits[idx] = 0

        def restore(first=False):
            if not first:
                t.insert(v, rows)
            t.assign_plane(1, v, acc)
            for s in range(0, args.keys, mb):
                t.set_hits(keys[s:s + mb], hits[s:s + mb])

        restore(first=True)
        ts = {f: [] for f in forms}
        for rep in range(args.reps + 2):      # the first two rounds warm up
            for f, fn in forms.items():       # the forms take turns
                us, m = timed(lambda: fn(n))
                assert m == n and t.size() == args.keys - n, (f, m)
                restore()
                if rep >= 2:
                    ts[f].append(us)
        for f, vs in ts.items():
            med = statistics.median(vs)
            results[f"{n} victims, {f}"] = {"median_us": med, "min_us": min(vs), "max_us": max(vs), "scan_GBps": scan_bytes / med / 1e3}
    assert t.status() == 0 and t.size() == args.keys
    print(f"dim {DIM}, Adagrad, {args.keys} keys in {t.capacity} slots, rows in {args.memory} memory; key + counter planes {scan_bytes / 1e6:.0f} MB; "
          f"{args.reps} timed calls per row")
    print("| case | median us | min .. max us | GB/s of key + counter planes per call |")
    print("|---|---|---|---|")
    for row, r in results.items():
        print(f"| {row} | {r['median_us']:.1f} | {r['min_us']:.1f} .. {r['max_us']:.1f} | {r['scan_GBps']:.0f} |")
    print("RESULT " + json.dumps(results), flush=True)


if __name__ == "__main__":
    main()
