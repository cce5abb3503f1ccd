"""Publish (SPEC.md §3 "Publish"): mee_publish_changed against the composition it replaces, on one MI355X.  Numbers go to profiles/publish.md.

  table    a --keys-key Adagrad table of dim 64 and a serving copy of it (bf16 rows, then fp32 rows without optimizer); a change log of N keys, nine
           tenths of them keys the trainer holds (upserts: the serving copy holds them too, their rows are overwritten), one tenth keys it does not
           hold (removals: put back into the serving copy, untimed, in front of every timed run, so that every run really removes them);
           N = 1K / 64K / 1M.  Forms: `publish` = ChangeLog.publish (one library call, two launches, no read-back) and `composition` =
           iter_changed(with_state=False) + insert + remove in max_batch chunks (what the tree had before), both ended by one device synchronise.
  group    26 tables x 4096 changed keys: TableGroup.publish_to(check=False) against 26 ChangeLog.publish calls and against 26 compositions.

The forms take turns inside one loop; the whole loop runs --passes times; reported: per pass the median of --reps runs, and the spread between passes.

usage: python tools/publish_bench.py table|group [--keys 10000000] [--reps 7] [--passes 2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["table", "group"])
ap.add_argument("--keys", type=int, default=10_000_000)
ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 10, 1 << 16, 1 << 20])
ap.add_argument("--group-tables", type=int, default=26)
ap.add_argument("--group-keys", type=int, default=200_000)
ap.add_argument("--group-changed", type=int, default=4096)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--passes", type=int, default=2)
args = ap.parse_args()
DIM, MB = 64, 1 << 20


def trainer(n_keys, dev, seed=1):
    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, synth
    t = LookupTable(int(n_keys / 0.75), DIM, device=dev, optimizer=OPT_ADAGRAD, max_batch=MB, initial_accumulator=0.1)
    for s in range(0, n_keys, MB):
        k = synth.keys_t(seed, s, min(MB, n_keys - s), dev)
        t.insert(k, synth.rows_t(k, DIM, 2))
    return t


def serving_of(t, bf16):
    import torch

    from meepoembedding_amd import LookupTable
    d = LookupTable(t.capacity, DIM, device=t.device, max_batch=MB, value_dtype=torch.bfloat16 if bf16 else torch.float32)
    for k, v, _, _ in t.iter_export(1 << 22, with_state=False):
        d.import_(k, v)
    return d


def chunks(x, n=MB):
    return [x[s:s + n] for s in range(0, x.shape[0], n)]


def compose(t, log, d):
    for k, v, _, _, gone in log.iter_changed(t, with_state=False):
        for kc, vc in zip(chunks(k), chunks(v)):
            d.insert(kc, vc)
        for gc in chunks(gone):
            d.remove(gc)


def changed_keys(n_keys, n, dev, seed):
    """-> (the keys to note, the removals among them): 9/10 drawn from the trainer's keys, 1/10 keys of another stream it does not hold"""
    import torch

    from meepoembedding_amd import synth
    n_gone = n // 10
    idx = torch.randperm(n_keys, device=dev)[: n - n_gone]
    present = synth.mix64_t((idx + 1) * synth._s64(synth._GOLDEN) + synth._s64(seed))   # keys_t(seed, ...) by index
    gone = synth.keys_t(1000 + seed, 0, n_gone, dev)
    return torch.cat([present, gone])[torch.randperm(n, device=dev)], gone


def race(dev, forms, restore):
    """forms: name -> callable; restore(): untimed, in front of every timed run -> {name: {pass medians, spread}} in microseconds"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    medians = {f: [] for f in forms}
    for _ in range(args.passes):
        ts = {f: [] for f in forms}
        for rep in range(args.reps + 1):           # the first round warms up
            for f, fn in forms.items():            # the forms take turns
                restore()
                torch.cuda.synchronize(dev)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize(dev)
                if rep:
                    ts[f].append(e0.elapsed_time(e1) * 1e3)
        for f in forms:
            medians[f].append(statistics.median(ts[f]))
    return {f: {"pass_median_us": [round(m, 1) for m in ms], "us": round(statistics.mean(ms), 1),
                "pass_spread_pct": round(100.0 * (max(ms) - min(ms)) / min(ms), 1)} for f, ms in medians.items()}


def with_ratios(r, base="publish"):
    for f in r:
        if f != base:
            r[f]["over_" + base] = round(r[f]["us"] / r[base]["us"], 2)
    return r


def bench_table(dev):
    import torch

    from meepoembedding_amd import synth
    from meepoembedding_amd.changes import ChangeLog
    t = trainer(args.keys, dev)
    res = {}
    for rows in ("bf16", "fp32"):
        d = serving_of(t, rows == "bf16")
        for n in args.sizes:
            noted, gone = changed_keys(args.keys, n, dev, seed=1)
            gone_rows = synth.rows_t(gone, DIM, 3)
            log = ChangeLog(2 * n, dev)
            for c in chunks(noted):
                log.note(c)
            assert log.size() == n and not log.invalid

            def restore():
                for kc, vc in zip(chunks(gone), chunks(gone_rows)):
                    d.insert(kc, vc)

            r = with_ratios(race(dev, {"publish": lambda: log.publish(t, d), "composition": lambda: compose(t, log, d)}, restore))
            restore()
            counts = log.publish(t, d).tolist()
            assert counts == [n - gone.numel(), gone.numel(), 0, 0], counts
            r["log_slots"] = log.capacity
            res[f"{rows} rows, {n} changed keys"] = r
            print(f"{rows} {n}: {json.dumps(r)}", flush=True)
        assert d.status() == 0 and d.size() == args.keys
        d.close()
        del d
        torch.cuda.empty_cache()
    return res


def bench_group(dev):
    import torch

    from meepoembedding_amd import TableGroup, synth
    nt, n = args.group_tables, args.group_changed
    tables = [trainer(args.group_keys, dev, seed=1) for _ in range(nt)]
    g = TableGroup(tables)
    g.track_changes(2 * n)
    serving = g.serving_copy()
    gone, gone_rows = [], []
    for j, t in enumerate(tables):
        noted, go = changed_keys(args.group_keys, n, dev, seed=1)
        t.change_log.note(noted)
        gone.append(go)
        gone_rows.append(synth.rows_t(go, DIM, 3))

    def restore():
        for j in range(nt):
            serving.tables[j].insert(gone[j], gone_rows[j])

    def singles():
        for j, t in enumerate(tables):
            t.change_log.publish(t, serving.tables[j])

    def compositions():
        for j, t in enumerate(tables):
            compose(t, t.change_log, serving.tables[j])

    r = with_ratios(race(dev, {"group publish": lambda: g.publish_to(serving, check=False), "26 publishes": singles, "26 compositions": compositions}, restore),
                    base="group publish")
    restore()
    n_gone = gone[0].numel()
    assert g.publish_to(serving) == [(n - n_gone, n_gone, 0)] * nt
    return {f"{nt} tables x {n} changed keys": r}


def main():
    import torch
    assert torch.cuda.is_available(), "publish_bench.py measures on the GPU: there is nothing to report without one"
    dev = torch.device("cuda", 0)
    res = {"table": bench_table, "group": bench_group}[args.what](dev)
    print("RESULT " + json.dumps({args.what: res, "keys": args.keys if args.what == "table" else args.group_keys, "dim": DIM, "reps": args.reps,
                                  "passes": args.passes}), flush=True)


if __name__ == "__main__":
    main()
