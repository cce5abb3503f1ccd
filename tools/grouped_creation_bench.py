"""The two grouped creation passes no other tool times (profiles/grouped_creation.md): the pooled lookup with insert_missing over

    tiered   a collection of hot/cold pairs   TieredTableGroup.find_pooled(insert_missing=True)   found pass, ensure_tiered_grouped_kernel, pooled launch
    mixed    a mixed-width collection         MixedTableGroup.find_pooled(insert_missing=True)    mixed_locate_kernel, mixed_ensure_kernel, pooled launch

on the collection shape of tools/group_admission_bench.py — 26 tables, 2048 ids per table and call, in 256 bags of 8 — dim 64 for the pairs, dims
32 / 64 / 128 in turn for the mixed collection.  Two states of the batch: every id stored (the creation launch leaves at its first wave-uniform
test), and a tenth new per call (every call gets ids nobody has asked for before, drawn from a counter; the tables are sized so that all ids created
over the whole run leave them under half full).  The pairs' new keys go to their hot tables; their cold tables hold keys of their own.

Method (group_admission_bench.py's): the rows of a state take turns in chunks of CHUNK calls inside one loop, a chunk is timed by the host clock
around its calls and a device synchronise, PASSES passes; a row's spread is its pass-to-pass difference.  To compare two builds of the library run
the tool once per build (MEE_LIB_PATH) and compare the rows.
Run on the GPU: python tools/grouped_creation_bench.py [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, MixedTableGroup, TieredTableGroup  # noqa: E402
from meepoembedding_amd.tiered import TieredLookupTable  # noqa: E402

N_TABLES, IDS, BAG, VOCAB, CAPACITY, COLD_KEYS = 26, 2048, 8, 100_000, 1 << 19, 10_000
MIXED_DIMS = (32, 64, 128)
ABSENT = IDS // 10
CHUNK, CHUNKS, PASSES, ROTATE = 10, 10, 2, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)

    def table(dim, j, capacity=CAPACITY):
        return LookupTable(capacity, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initializer=INIT_UNIFORM, init_scale=0.05, init_seed=j)

    def store(t, first, count):
        for start in range(first, first + count, 4096):
            t.find_or_insert(torch.arange(start, min(start + 4096, first + count), dtype=torch.int64, device=dev))

    hot = [table(64, j) for j in range(N_TABLES)]
    cold = [table(64, 100 + j, 1 << 15) for j in range(N_TABLES)]
    mixed = [table(MIXED_DIMS[j % 3], j) for j in range(N_TABLES)]
    for t in hot + mixed:
        store(t, 0, VOCAB)   # the stored vocabulary: ids 0 .. VOCAB - 1 in every table
    for t in cold:
        store(t, 1 << 40, COLD_KEYS)
    groups = {"tiered": TieredTableGroup([TieredLookupTable(h, c, hot_key_limit=1 << 60) for h, c in zip(hot, cold)]), "mixed": MixedTableGroup(mixed)}
    n = N_TABLES * IDS
    bag_offsets = torch.arange(0, n + 1, BAG, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    where = torch.randperm(IDS, device=dev, generator=gen)[:ABSENT]
    fresh = {name: VOCAB for name in groups}   # per collection: the next id nobody has asked for
    found = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(ROTATE)]

    def stored_batch():
        return torch.randint(0, VOCAB, (N_TABLES, IDS), dtype=torch.int64, device=dev, generator=gen)

    present = [stored_batch().reshape(-1).contiguous() for _ in range(ROTATE)]

    def new_ids(name):
        b = stored_batch()
        b[:, where] = fresh[name] + torch.arange(ABSENT, dtype=torch.int64, device=dev)
        fresh[name] += ABSENT
        return b.reshape(-1).contiguous()

    states = [("every id stored", lambda name, r: present[r % ROTATE]), ("a tenth new per call", lambda name, r: new_ids(name))]
    result = {"tables": N_TABLES, "ids_per_table": IDS, "ids_per_bag": BAG, "stored_per_table": VOCAB, "capacity": hot[0].capacity, "mixed_dims": list(MIXED_DIMS),
              "calls_per_row_and_pass": CHUNK * CHUNKS, "states": []}
    for title, batch_of in states:
        for name, g in groups.items():   # warm-up: every row of the state, every rotating buffer
            for r in range(ROTATE):
                g.find_pooled(batch_of(name, r), bag_offsets, "sum", found=found[r], insert_missing=True)
        torch.cuda.synchronize(dev)
        us = {name: [] for name in groups}
        for _ in range(PASSES):
            total = {name: 0.0 for name in groups}
            for c in range(CHUNKS):
                for name, g in groups.items():
                    batches = [batch_of(name, c * CHUNK + i) for i in range(CHUNK)]   # made before the clock starts
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for i, keys in enumerate(batches):
                        g.find_pooled(keys, bag_offsets, "sum", found=found[i % ROTATE], insert_missing=True)
                    torch.cuda.synchronize(dev)
                    total[name] += time.perf_counter() - t0
            for name in total:
                us[name].append(total[name] / (CHUNK * CHUNKS) * 1e6)
        entry = {"state": title, "us_per_call": us, "spread_us": {name: abs(v[0] - v[1]) for name, v in us.items()}}
        print(f"\n{title}")
        for name, v in us.items():
            print(f"  {name:8s} " + " / ".join(f"{x:8.2f}" for x in v) + f"  us per call (pass 1 / 2), spread {entry['spread_us'][name]:.2f} us")
        result["states"].append(entry)
    assert all(t.status() == 0 for t in hot + cold + mixed)
    assert all(t.size() == VOCAB + fresh["tiered"] - VOCAB for t in hot) and all(t.size() == fresh["mixed"] for t in mixed) and all(t.size() == COLD_KEYS for t in cold)
    result["fill_after"] = max(t.size() for t in hot + mixed) / hot[0].capacity
    print(f"\nfullest table after the run: {result['fill_after']:.3f} of its capacity")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
