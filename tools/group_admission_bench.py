"""Admission over a table group against the per-table loop (profiles/group_admission.md): the collection of examples/recsys_collection.py —
26 tables, dim 64, 2048 ids per table and call — served by

    grouped   TableGroup.find_or_insert(min_count=)           one operator, three launches
    loop      26 x LookupTable.find_or_insert(min_count=)     the per-table operator on the same tables, four launches each
    plain     TableGroup.find_or_insert()                      no admission, two launches: grouped - plain = what admission costs

in three states of the batch: every id stored; a tenth absent and below the threshold (counted, not created: the threshold is 2^32 - 1, so the same
batches can be served for ever); a tenth absent and admitted in that call (threshold 1; every call of every row gets ids nobody has asked for before,
drawn from a counter, and the tables are sized so that all ids created over the whole run leave them under half full — nothing is removed between
calls).  `plain` has no counted-not-created state — without admission the absent tenth would be created by its first call — so it is timed in the
other two.

Method (as profiles/int8_rows.md): the rows of a state take turns in chunks of CHUNK calls inside one loop, a chunk is timed by the host clock around
its calls and a device synchronise, PASSES passes; the spread of a comparison is the largest pass-to-pass difference of the rows compared.
Run on the GPU: python tools/group_admission_bench.py [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TableGroup  # noqa: E402

N_TABLES, DIM, IDS, VOCAB, CAPACITY = 26, 64, 2048, 100_000, 1 << 19
ABSENT = IDS // 10
CHUNK, CHUNKS, PASSES, ROTATE = 10, 10, 2, 6
NEVER = 2**32 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tables = [LookupTable(CAPACITY, DIM, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, admission=True, initializer=INIT_UNIFORM, init_scale=0.05,
                          init_seed=j) for j in range(N_TABLES)]
    group = TableGroup(tables)
    n = N_TABLES * IDS
    offsets = torch.arange(0, n + 1, IDS, dtype=torch.int64, device=dev)
    bounds = [(j * IDS, (j + 1) * IDS) for j in range(N_TABLES)]
    for start in range(0, VOCAB, IDS):   # the stored vocabulary: ids 0 .. VOCAB - 1 in every table
        ids = torch.arange(start, min(start + IDS, VOCAB), dtype=torch.int64, device=dev)
        ids = torch.cat([ids, ids[:IDS - ids.numel()]]) if ids.numel() < IDS else ids
        group.find_or_insert(ids.repeat(N_TABLES), offsets)
    assert all(t.size() == VOCAB for t in tables)
    gen = torch.Generator(device=dev).manual_seed(3)
    outs = [(torch.empty((n, DIM), device=dev), torch.empty(n, dtype=torch.uint8, device=dev)) for _ in range(ROTATE)]
    where = torch.randperm(IDS, device=dev, generator=gen)[:ABSENT]
    fresh = [VOCAB + ROTATE * ABSENT]   # the next id nobody has asked for (the ids below it: the absent tenths of the counted-not-created batches)

    def stored_batch():
        return torch.randint(0, VOCAB, (N_TABLES, IDS), dtype=torch.int64, device=dev, generator=gen)

    def with_absent(first):
        b = stored_batch()
        b[:, where] = first + torch.arange(ABSENT, dtype=torch.int64, device=dev)
        return b.reshape(-1).contiguous()

    present = [stored_batch().reshape(-1).contiguous() for _ in range(ROTATE)]
    counted = [with_absent(VOCAB + r * ABSENT) for r in range(ROTATE)]

    def new_ids(_):
        fresh[0] += ABSENT
        return with_absent(fresh[0] - ABSENT)

    def grouped(min_count):
        return lambda keys, out, found: group.find_or_insert(keys, offsets, out=out, found=found, min_count=min_count)

    def loop(min_count):
        def run(keys, out, found):
            for t, (s, e) in zip(tables, bounds):
                t.find_or_insert(keys[s:e], out=out[s:e], found=found[s:e], min_count=min_count)
        return run

    def plain(keys, out, found):
        group.find_or_insert(keys, offsets, out=out, found=found)

    states = [
        ("every id stored", lambda r: present[r % ROTATE], [("grouped", grouped(2)), ("loop", loop(2)), ("plain", plain)]),
        ("a tenth absent, counted and not created", lambda r: counted[r % ROTATE], [("grouped", grouped(NEVER)), ("loop", loop(NEVER))]),
        ("a tenth absent, admitted in the call", new_ids, [("grouped", grouped(1)), ("loop", loop(1)), ("plain", plain)]),
    ]
    result = {"tables": N_TABLES, "dim": DIM, "ids_per_table": IDS, "stored_per_table": VOCAB, "capacity": tables[0].capacity, "calls_per_row_and_pass": CHUNK * CHUNKS,
              "states": []}
    for title, batch_of, rows in states:
        for name, fn in rows:   # warm-up: every row of the state, every rotating buffer
            for r in range(ROTATE):
                fn(batch_of(r), *outs[r])
        torch.cuda.synchronize(dev)
        us = {name: [] for name, _ in rows}
        for _ in range(PASSES):
            total = {name: 0.0 for name, _ in rows}
            for c in range(CHUNKS):
                for name, fn in rows:
                    batches = [batch_of(c * CHUNK + i) for i in range(CHUNK)]   # made before the clock starts
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for i, keys in enumerate(batches):
                        fn(keys, *outs[i % ROTATE])
                    torch.cuda.synchronize(dev)
                    total[name] += time.perf_counter() - t0
            for name in total:
                us[name].append(total[name] / (CHUNK * CHUNKS) * 1e6)
        entry = {"state": title, "us_per_call": us, "comparisons": {}}
        print(f"\n{title}")
        for name, v in us.items():
            print(f"  {name:8s} " + " / ".join(f"{x:8.2f}" for x in v) + "  us per call (pass 1 / 2)")
        for other in [name for name, _ in rows if name != "grouped"]:
            spread = max(abs(us[k][0] - us[k][1]) for k in ("grouped", other))
            a, b = sum(us["grouped"]) / PASSES, sum(us[other]) / PASSES
            verdict = "within spread" if abs(a - b) <= spread else ("grouped faster" if a < b else "grouped SLOWER")
            entry["comparisons"][other] = {"other_over_grouped": b / a, "difference_us": b - a, "spread_us": spread, "verdict": verdict}
            print(f"  {other} / grouped = {b / a:.3f}x, {other} - grouped = {b - a:.2f} us, spread {spread:.2f} us: {verdict}")
        result["states"].append(entry)
    result["fill_after"] = max(t.size() for t in tables) / tables[0].capacity
    print(f"\nfullest table after the run: {result['fill_after']:.3f} of its capacity")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
