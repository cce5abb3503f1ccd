"""The unpooled lookups over a COLLECTION of hot/cold pairs (TieredTableGroup.find / find_or_insert, mee_group_find_tiered, mee_group_find_or_insert_tiered):
26 members, dim 64, a jagged batch of 2048 ids per table, every member a hot/cold pair (hot tier in HBM, cold rows in pinned host memory); uniform keys,
every lookup hot or a tenth of them cold.  Sides, per placement and operator:
  group  find: ONE mee_group_find_tiered launch;  find_or_insert: mee_group_find_or_insert_tiered, two launches
  loop   find: mee_find + mee_find_missing per member (52 launches);  find_or_insert: + mee_find_or_insert_missing per member (78 launches) —
         TieredLookupTable.find / find_or_insert member by member, what the collection paid before
  flat   find only, all-hot placement only: ONE mee_find_grouped launch over the 26 hot tables — what the tier check costs per launch
Every id of the batch is stored, so find_or_insert creates nothing: the steady state of a trained vocabulary (its creation launch still runs).
Every side is called through ctypes with arguments prepared once, so that the host adds as little as it can to either.

A side is timed in chunks (device events around `reps` calls); a process times ONE side (--side), so that the loop can run on another build of the
library (MEE_LIB_PATH, MEE_LIB_OLDER_BUILD=1: the parent commit's).  Without --side the tool is the driver: it starts one fresh child process per side
and pass, the sides taking turns, `--passes` passes, and prints per row the median of each pass, the pass-to-pass spread and the ratio loop / group.
usage: python tools/tiered_group_find_bench.py [--loop-lib PATH] [--passes 2] [--chunks 7] [--reps 40] [--hot KEYS] [--cold KEYS]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--side", choices=["group", "loop", "flat"], default=None)
ap.add_argument("--loop-lib", default=None, help="driver: the library the loop side runs on (default: this tree's)")
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--chunks", type=int, default=7)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--hot", type=int, default=200_000, help="hot keys per member")
ap.add_argument("--cold", type=int, default=50_000, help="cold keys per member")
args = ap.parse_args()
N_TABLES, DIM, PER_TABLE = 26, 64, 2048


def child():
    import torch

    from meepoembedding_amd import LookupTable, TableGroup, _lib, synth
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    g = torch.Generator(device=dev)

    def fill(table, stream, count):
        k = synth.keys_t(stream, 0, count, dev)
        table.insert(k, synth.rows_t(k, DIM, 2))
        return k

    hots, colds, hot_keys, cold_keys = [], [], [], []
    for j in range(N_TABLES):
        hots.append(LookupTable(int(args.hot / 0.75), DIM, device=dev, max_batch=max(args.hot, args.cold)))
        hot_keys.append(fill(hots[-1], 100 + j, args.hot))
        if args.side != "flat":
            colds.append(LookupTable(int(args.cold / 0.75), DIM, device=dev, max_batch=max(args.hot, args.cold), value_memory=_lib.MEM_HOST_PINNED))
            cold_keys.append(fill(colds[-1], 200 + j, args.cold))
    torch.cuda.synchronize(dev)
    if args.side == "group":
        hot_group, cold_group = TableGroup(hots), TableGroup(colds)
    elif args.side == "flat":
        flat_group = TableGroup(hots)

    n = N_TABLES * PER_TABLE
    off = torch.arange(N_TABLES + 1, dtype=torch.int64, device=dev) * PER_TABLE
    seg = off.tolist()
    results = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for row_seed, (placement, hot_share) in enumerate((("all hot", 1.0), ("90 % hot", 0.9))):
        if args.side == "flat" and hot_share < 1.0:
            continue
        g.manual_seed(100 + row_seed)      # every side draws the same keys
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        for j in range(N_TABLES):
            k = hot_keys[j][(torch.rand(PER_TABLE, device=dev, generator=g) * args.hot).long().clamp(0, args.hot - 1)]
            if hot_share < 1.0:
                cold = torch.rand(PER_TABLE, device=dev, generator=g) >= hot_share
                k = torch.where(cold, cold_keys[j][(torch.rand(PER_TABLE, device=dev, generator=g) * args.cold).long().clamp(0, args.cold - 1)], k)
            keys[seg[j]:seg[j + 1]] = k
        out = torch.empty((n, DIM), device=dev)
        found = torch.empty(n, dtype=torch.uint8, device=dev)
        calls = {}
        if args.side == "group":
            a = (hot_group._h, cold_group._h, keys.data_ptr(), off.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, found.data_ptr())
            calls["find"] = lambda a=a: L.mee_group_find_tiered(*a, 0, None)
            calls["find_or_insert"] = lambda a=a: L.mee_group_find_or_insert_tiered(*a, None, 0, None)
        elif args.side == "flat":
            a = (flat_group._h, keys.data_ptr(), off.data_ptr(), n, out.data_ptr(), found.data_ptr(), None)
            calls["find"] = lambda a=a: L.mee_find_grouped(*a)
        else:
            per = [(keys.data_ptr() + 8 * seg[j], PER_TABLE, out.data_ptr() + 4 * DIM * seg[j], found.data_ptr() + seg[j], None) for j in range(N_TABLES)]

            def loop_find(per=per):
                for j, p in enumerate(per):
                    L.mee_find(hots[j]._h, *p)
                    L.mee_find_missing(colds[j]._h, *p)

            def loop_foi(per=per):
                for j, p in enumerate(per):
                    L.mee_find(hots[j]._h, *p)
                    L.mee_find_missing(colds[j]._h, *p)
                    L.mee_find_or_insert_missing(hots[j]._h, *p)
            calls["find"], calls["find_or_insert"] = loop_find, loop_foi
        for op, call in calls.items():
            for _ in range(10):
                rc = call()
            assert args.side == "loop" or rc == 0, (op, rc)
            torch.cuda.synchronize(dev)
            ts = []
            for _ in range(args.chunks):
                e0.record()
                for _ in range(args.reps):
                    call()
                e1.record()
                torch.cuda.synchronize(dev)
                ts.append(e0.elapsed_time(e1) * 1e3 / args.reps)
            results[f"{op}, {placement}"] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "keys": n,
                                              "checksum": float(out.double().sum()), "found": int(found.sum())}
    print("RESULT " + json.dumps(results), flush=True)


def driver():
    table = {}      # row -> side -> [median per pass]
    sums = {}
    for p in range(args.passes):
        for side in ("loop", "group", "flat"):      # the sides take turns, a fresh process each
            env = dict(os.environ)
            if side == "loop" and args.loop_lib:
                env.update(MEE_LIB_PATH=os.path.abspath(args.loop_lib), MEE_LIB_OLDER_BUILD="1")
            cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--chunks", str(args.chunks), "--reps", str(args.reps),
                   "--hot", str(args.hot), "--cold", str(args.cold)]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            line = [x for x in res.stdout.splitlines() if x.startswith("RESULT ")]
            if res.returncode != 0 or not line:
                print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"side {side}, pass {p + 1} failed with exit status {res.returncode}")
            for row, r in json.loads(line[0][7:]).items():
                table.setdefault(row, {}).setdefault(side, []).append(r["median_us"])
                if side != "flat":
                    sums.setdefault(row, set()).add((r["checksum"], r["found"]))
                print(f"pass {p + 1} {side:5s} {row}: median {r['median_us']:.1f} us (chunks {r['min_us']:.1f} .. {r['max_us']:.1f}), {r['keys']} keys", flush=True)
    print(f"\n{N_TABLES} members, dim {DIM}, {PER_TABLE} ids per table, {args.hot} hot + {args.cold} cold keys per member; {args.passes} passes x {args.chunks} chunks x {args.reps} calls; "
          f"loop on {'the library at ' + args.loop_lib if args.loop_lib else 'this build'}")
    print("| operator, placement | loop us (per pass) | group us (per pass) | flat us (per pass) | larger pass-to-pass spread | loop / group | faster by more than the spread |")
    print("|---|---|---|---|---|---|---|")
    for row, sides in table.items():
        assert len(sums[row]) == 1, f"{row}: the loop and the group disagree on the rows or the found mask: {sums[row]}"
        spread = {s: (max(v) - min(v)) / statistics.mean(v) for s, v in sides.items()}
        lo, gr = statistics.mean(sides["loop"]), statistics.mean(sides["group"])
        worst = max(spread["loop"], spread["group"])
        fmt = lambda v: " / ".join(f"{x:.1f}" for x in v)  # noqa: E731
        print(f"| {row} | {fmt(sides['loop'])} | {fmt(sides['group'])} | {fmt(sides['flat']) if 'flat' in sides else '—'} | {worst * 100:.1f} % | {lo / gr:.2f} | "
              f"{'yes' if (lo - gr) / lo > worst else 'NO'} |")


if __name__ == "__main__":
    child() if args.side else driver()
