"""Tier migration: the native move (mee_move / mee_group_move) against the operator sequence it replaces (find, insert, find_plane / assign_plane,
remove — TieredLookupTable._move_by_operators, the same code and kernels as before the move existed), on the same tree and in the same process, the two
forms taking turns.

Part 1, one pair: dim 64, Adagrad, a hot table in HBM and a cold table in pinned host memory of --keys keys each.  A batch of hot keys is demoted
(HBM -> host) and promoted back (host -> HBM), so the pair is in the same state before every timed call; batches of 1K, 64K and 1M keys (those within
max_batch).  A call is timed by device events around the whole Python call, its read-back of the count included; reported: the median and the
min .. max of --reps calls, and the bytes a key moves, 8 + 2 * P * 4 * dim (P planes: read once, written once), over the median.
Part 2, a collection: 26 pairs, --per-pair keys per pair demoted and promoted back — the moves of one TieredTableGroup.rebalance() — as two grouped moves
(TieredTableGroup._move_lists) against the per-pair loop, native and by operators.

--cold-memory hbm puts the cold tables into HBM as well: the same calls without the link.

usage: python tools/tier_move_bench.py [--keys 10000000] [--reps 21] [--per-pair 4000] [--skip-group] [--cold-memory host|hbm]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=10_000_000, help="keys in the hot table and in the cold table")
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--per-pair", type=int, default=4000)
ap.add_argument("--skip-group", action="store_true")
ap.add_argument("--cold-memory", choices=["host", "hbm"], default="host", help="hbm: the cold tables live in HBM too (what the kernels do without the link)")
args = ap.parse_args()
DIM, PLANES, N_PAIRS = 64, 2, 26
KEY_BYTES = 8 + 2 * PLANES * 4 * DIM


def main():
    import torch

    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, _lib, synth
    from meepoembedding_amd.tiered import TieredLookupTable, TieredTableGroup
    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3, r

    def make_pair(n_hot, n_cold, stream, max_batch):
        hot = LookupTable(int(n_hot / 0.75), DIM, device=dev, optimizer=OPT_ADAGRAD, max_batch=max_batch, track_hits=True)
        cold = LookupTable(int((n_cold + min(n_hot, max_batch)) / 0.75), DIM,   # room for one batch of demoted keys
                           device=dev, optimizer=OPT_ADAGRAD, max_batch=max_batch,
                           value_memory=_lib.MEM_HBM if args.cold_memory == "hbm" else _lib.MEM_HOST_PINNED, track_hits=True)
        hk, ck = synth.keys_t(stream, 0, n_hot, dev), synth.keys_t(stream + 1000, 0, n_cold, dev)
        for t, k in ((hot, hk), (cold, ck)):
            for s in range(0, k.numel(), max_batch):
                t.insert(k[s:s + max_batch], synth.rows_t(k[s:s + max_batch], DIM, 2))
        return TieredLookupTable(hot, cold, hot_key_limit=n_hot), hk

    results = {}
    # ---- part 1: one pair ----
    max_batch = 1 << 20
    pair, hk = make_pair(args.keys, args.keys, 1, max_batch)
    forms = {"move": pair._move, "operators": pair._move_by_operators}
    for n in (1 << 10, 1 << 16, 1 << 20):
        if n > min(max_batch, args.keys):
            continue
        batch = hk[torch.randperm(args.keys, device=dev)[:n]].contiguous()
        ts = {(f, d): [] for f in forms for d in ("demote", "promote")}
        for rep in range(args.reps + 2):    # the first two rounds warm up
            for f, fn in forms.items():     # the forms take turns
                t_d, m_d = timed(lambda: fn(pair.hot, pair.cold, batch))
                t_p, m_p = timed(lambda: fn(pair.cold, pair.hot, batch))
                assert m_d == m_p == n, (f, m_d, m_p)
                if rep >= 2:
                    ts[(f, "demote")].append(t_d); ts[(f, "promote")].append(t_p)
        for (f, d), v in ts.items():
            med = statistics.median(v)
            results[f"pair {d} {n} keys, {f}"] = {"median_us": med, "min_us": min(v), "max_us": max(v), "GBps": n * KEY_BYTES / med / 1e3}
    assert pair.hot.status() == 0 and pair.cold.status() == 0
    pair.hot.close(); pair.cold.close()
    # ---- part 2: the moves of a rebalance over 26 pairs ----
    if not args.skip_group:
        made = [make_pair(200_000, 50_000, 10 + 2 * j, 1 << 18) for j in range(N_PAIRS)]
        pairs = [m[0] for m in made]
        group = TieredTableGroup(pairs)
        lists = [m[1][: args.per_pair].contiguous() for m in made]
        forms = {
            "grouped move": lambda s, d: group._move_lists(group.hot_group if s == "hot" else group.cold_group, group.cold_group if s == "hot" else group.hot_group, lists),
            "loop of moves": lambda s, d: [p._move(getattr(p, s), getattr(p, d), k) for p, k in zip(pairs, lists)],
            "loop of operators": lambda s, d: [p._move_by_operators(getattr(p, s), getattr(p, d), k) for p, k in zip(pairs, lists)],
        }
        ts = {f: [] for f in forms}
        for rep in range(args.reps + 2):
            for f, fn in forms.items():
                t_d, m_d = timed(lambda: fn("hot", "cold"))
                t_p, m_p = timed(lambda: fn("cold", "hot"))
                assert list(m_d) == list(m_p) == [args.per_pair] * N_PAIRS, f
                if rep >= 2:
                    ts[f].append(t_d + t_p)
        for f, v in ts.items():
            med = statistics.median(v)
            results[f"{N_PAIRS} pairs, {args.per_pair} keys each out and back, {f}"] = {"median_us": med, "min_us": min(v), "max_us": max(v),
                                                                                      "GBps": 2 * N_PAIRS * args.per_pair * KEY_BYTES / med / 1e3}
    print(f"dim {DIM}, Adagrad ({PLANES} planes, {KEY_BYTES} bytes moved per key), {args.keys} keys per tier, cold tables in {args.cold_memory} memory; {args.reps} timed calls per row")
    print("| case | median us | min .. max us | GB/s of moved bytes |")
    print("|---|---|---|---|")
    for row, r in results.items():
        print(f"| {row} | {r['median_us']:.1f} | {r['min_us']:.1f} .. {r['max_us']:.1f} | {r['GBps']:.1f} |")
    print("RESULT " + json.dumps(results), flush=True)


if __name__ == "__main__":
    main()
