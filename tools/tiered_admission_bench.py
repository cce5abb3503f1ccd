"""Admission over a collection of hot/cold pairs against the per-pair loop and against the non-admitting call (profiles/tiered_admission.md): the
shape of profiles/group_admission.md — 26 pairs, dim 64, 2048 ids per pair and call — hot tables in HBM, cold rows in pinned host memory, served by

    grouped   TieredTableGroup.find_or_insert(min_count=)            mee_group_find_or_insert_admit_tiered, three launches
    loop      26 x TieredLookupTable.find_or_insert(min_count=)      per pair: find, find_missing, count, decide, create — five launches each
    plain     TieredTableGroup.find_or_insert()                      no admission, two launches: grouped - plain = what admission costs

in four states of the batch: every id stored hot; a tenth of every segment stored cold; a tenth absent and below the threshold (2^32 - 1: counted,
never created, so the same batches serve for ever; no `plain` row — without admission its first call would create them); a tenth absent and admitted
in the call (threshold 1; every call of every row gets ids nobody has asked for before, and the hot tables are sized so that the whole run leaves
them at 0.6 of their capacity).  Then the pooled lookup with its creation pass, TieredTableGroup.find_pooled(insert_missing=True), with min_count (four
launches) and without (three), bags of 8 ids, in the all-hot state and with a tenth absent and created at first sight.

The pairs get a hot_key_limit nothing here reaches, so no call refreshes a hot table's size (a synchronisation): the host's placement bookkeeping is
the same list of additions in every row.

Method (as tools/group_admission_bench.py): the rows of a state take turns in chunks of CHUNK calls inside one loop, a chunk is timed by the host
clock around its calls and a device synchronise, PASSES passes; the spread of a comparison is the largest pass-to-pass difference of the rows compared.
Run on the GPU: python tools/tiered_admission_bench.py [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TieredLookupTable, TieredTableGroup, _lib  # noqa: E402

N_TABLES, DIM, IDS, VOCAB, COLD_VOCAB, CAPACITY, COLD_CAPACITY = 26, 64, 2048, 100_000, 20_000, 1 << 19, 1 << 16
TENTH = IDS // 10
BAG = 8
CHUNK, CHUNKS, PASSES, ROTATE = 10, 10, 2, 6
NEVER = 2**32 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    kw = dict(device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initializer=INIT_UNIFORM, init_scale=0.05)
    pairs = [TieredLookupTable(LookupTable(CAPACITY, DIM, admission=True, init_seed=j, **kw),
                               LookupTable(COLD_CAPACITY, DIM, init_seed=j, value_memory=_lib.MEM_HOST_PINNED, **kw), hot_key_limit=1 << 40) for j in range(N_TABLES)]
    group = TieredTableGroup(pairs)
    n = N_TABLES * IDS
    offsets = torch.arange(0, n + 1, IDS, dtype=torch.int64, device=dev)
    bag_offsets = torch.arange(0, n + 1, BAG, dtype=torch.int64, device=dev)
    bounds = [(j * IDS, (j + 1) * IDS) for j in range(N_TABLES)]
    for first, vocab, g in ((0, VOCAB, group.hot_group), (VOCAB, COLD_VOCAB, group.cold_group)):   # hot: ids 0 .. VOCAB - 1; cold: the COLD_VOCAB ids behind them
        for start in range(first, first + vocab, IDS):
            ids = torch.arange(start, min(start + IDS, first + vocab), dtype=torch.int64, device=dev)
            ids = torch.cat([ids, ids[:IDS - ids.numel()]]) if ids.numel() < IDS else ids
            g.find_or_insert(ids.repeat(N_TABLES), offsets)
    assert all(p.hot.size() == VOCAB and p.cold.size() == COLD_VOCAB for p in pairs)
    gen = torch.Generator(device=dev).manual_seed(3)
    outs = [(torch.empty((n, DIM), device=dev), torch.empty(n, dtype=torch.uint8, device=dev)) for _ in range(ROTATE)]
    pooled = [torch.empty((n // BAG, DIM), device=dev) for _ in range(ROTATE)]
    where = torch.randperm(IDS, device=dev, generator=gen)[:TENTH]
    first_absent = VOCAB + COLD_VOCAB
    fresh = [first_absent + ROTATE * TENTH]   # the next id nobody has asked for (the ids below it: the absent tenths of the counted-not-created batches)

    def stored_batch():
        return torch.randint(0, VOCAB, (N_TABLES, IDS), dtype=torch.int64, device=dev, generator=gen)

    def with_tenth(ids):
        b = stored_batch()
        b[:, where] = ids
        return b.reshape(-1).contiguous()

    def with_absent(first):
        return with_tenth(first + torch.arange(TENTH, dtype=torch.int64, device=dev))

    present = [stored_batch().reshape(-1).contiguous() for _ in range(ROTATE)]
    cold = [with_tenth(torch.randint(VOCAB, VOCAB + COLD_VOCAB, (N_TABLES, TENTH), dtype=torch.int64, device=dev, generator=gen)) for _ in range(ROTATE)]
    counted = [with_absent(first_absent + r * TENTH) for r in range(ROTATE)]

    def new_ids(_):
        fresh[0] += TENTH
        return with_absent(fresh[0] - TENTH)

    def grouped(min_count):
        return lambda keys, r: group.find_or_insert(keys, offsets, out=outs[r][0], found=outs[r][1], min_count=min_count)

    def loop(min_count):
        def run(keys, r):
            for p, (s, e) in zip(pairs, bounds):
                p.find_or_insert(keys[s:e], min_count=min_count)
        return run

    def plain(keys, r):
        group.find_or_insert(keys, offsets, out=outs[r][0], found=outs[r][1])

    def bags(min_count):
        return lambda keys, r: group.find_pooled(keys, bag_offsets, "sum", out=pooled[r], found=outs[r][1], insert_missing=True, min_count=min_count)

    unpooled = lambda c: [("grouped", grouped(c)), ("loop", loop(c)), ("plain", plain)]  # noqa: E731
    states = [
        ("every id stored, every lookup hot", lambda r: present[r % ROTATE], unpooled(2)),
        ("a tenth stored cold", lambda r: cold[r % ROTATE], unpooled(2)),
        ("a tenth absent, counted and not created", lambda r: counted[r % ROTATE], unpooled(NEVER)[:2]),
        ("a tenth absent, admitted in the call", new_ids, unpooled(1)),
        ("pooled, every id stored hot", lambda r: present[r % ROTATE], [("grouped", bags(2)), ("plain", bags(None))]),
        ("pooled, a tenth absent and created at first sight", new_ids, [("grouped", bags(1)), ("plain", bags(None))]),
    ]
    result = {"pairs": N_TABLES, "dim": DIM, "ids_per_pair": IDS, "hot_stored": VOCAB, "cold_stored": COLD_VOCAB, "hot_capacity": pairs[0].hot.capacity,
              "cold_capacity": pairs[0].cold.capacity, "bag": BAG, "calls_per_row_and_pass": CHUNK * CHUNKS, "states": []}
    for title, batch_of, rows in states:
        for name, fn in rows:   # warm-up: every row of the state, every rotating buffer
            for r in range(ROTATE):
                fn(batch_of(r), r)
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
                        fn(keys, i % ROTATE)
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
    result["fill_after"] = max(p.hot.size() for p in pairs) / pairs[0].hot.capacity
    assert all(p.cold.size() == COLD_VOCAB for p in pairs)   # nothing was created cold
    print(f"\nfullest hot table after the run: {result['fill_after']:.3f} of its capacity")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
