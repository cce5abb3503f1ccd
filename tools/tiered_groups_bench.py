"""Embedding bags over a COLLECTION of hot/cold pairs (TieredTableGroup, mee_group_find_pooled_tiered): the collection of examples/recsys_collection.py —
26 members, dim 64, 2048 bags per table — with every member a hot/cold pair (hot tier in HBM, cold rows in pinned host memory).
Rows of the table it prints, per bag shape (mean length 8: four bags per wave; mean length 20: a wave per bag), key stream (uniform, Zipf) and placement
(every lookup hot; 90 % of the lookups hot):
  group  ONE mee_group_find_pooled_tiered launch for the 26 x 2048 bags
  loop   26 mee_find_pooled_tiered launches, member by member (what the collection paid before)
  flat   ONE mee_group_find_pooled launch over 26 untiered tables holding the hot keys (all-hot placement only): what tier-awareness costs per launch
Every side is called through ctypes with arguments prepared once, so that the host adds as little as it can to either.

A side is timed in chunks (device events around `reps` calls); a process times ONE side (--side), so that the loop can run on another build of the
library (MEE_LIB_PATH, MEE_LIB_OLDER_BUILD=1: the parent commit's).  Without --side the tool is the driver: it starts one fresh child process per side
and pass, the sides taking turns, `--passes` passes, and prints per row the median of each pass, the pass-to-pass spread and the ratio loop / group.
usage: python tools/tiered_groups_bench.py [--loop-lib PATH] [--passes 2] [--chunks 7] [--reps 40] [--hot KEYS] [--cold KEYS]"""
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
N_TABLES, DIM, BPT = 26, 64, 2048
SHAPES = {"mean 8": (1, 15), "mean 20": (12, 28)}      # bag lengths drawn uniformly from [lo, hi]


def child():
    import torch

    from meepoembedding_amd import LookupTable, TableGroup, _lib, synth
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    g = torch.Generator(device=dev)
    g.manual_seed(5)

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

    def draw(n, vocab, zipf):
        u = torch.rand(n, device=dev, generator=g)
        if zipf:    # rank = floor(vocab ** u) - 1: log-uniform ranks, the Zipf law of exponent 1
            return (torch.exp(u.double() * float(torch.log(torch.tensor(float(vocab))))).long() - 1).clamp(0, vocab - 1)
        return (u * vocab).long().clamp(0, vocab - 1)

    results = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    row_seed = 100
    for shape, (lo, hi) in SHAPES.items():
        g.manual_seed(len(shape) + lo)      # every side draws the same bags and, per row, the same keys
        lens = torch.randint(lo, hi + 1, (N_TABLES * BPT,), device=dev, generator=g)
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        n = int(off[-1])
        seg = off[::BPT].tolist()
        for dist in ("uniform", "zipf"):
            for placement, hot_share in (("all hot", 1.0), ("90 % hot", 0.9)):
                row_seed += 1
                g.manual_seed(row_seed)
                if args.side == "flat" and hot_share < 1.0:
                    continue
                keys = torch.empty(n, dtype=torch.int64, device=dev)
                for j in range(N_TABLES):
                    m = seg[j + 1] - seg[j]
                    k = hot_keys[j][draw(m, args.hot, dist == "zipf")]
                    if hot_share < 1.0:
                        cold = torch.rand(m, device=dev, generator=g) >= hot_share
                        k = torch.where(cold, cold_keys[j][draw(m, args.cold, dist == "zipf")], k)
                    keys[seg[j]:seg[j + 1]] = k
                out = torch.empty((N_TABLES * BPT, DIM), device=dev)
                found = torch.empty(n, dtype=torch.uint8, device=dev)
                if args.side == "group":
                    a = (hot_group._h, cold_group._h, keys.data_ptr(), n, off.data_ptr(), BPT, out.data_ptr(), _lib.DTYPE_F32, found.data_ptr(), 0, 0, None)
                    call = lambda: L.mee_group_find_pooled_tiered(*a)  # noqa: E731
                elif args.side == "flat":
                    a = (flat_group._h, keys.data_ptr(), n, off.data_ptr(), BPT, out.data_ptr(), found.data_ptr(), None, 0, None)
                    call = lambda: L.mee_group_find_pooled(*a)  # noqa: E731
                else:
                    offs = [(off[j * BPT:(j + 1) * BPT + 1] - seg[j]).contiguous() for j in range(N_TABLES)]
                    per = [(hots[j]._h, colds[j]._h, keys.data_ptr() + 8 * seg[j], seg[j + 1] - seg[j], offs[j].data_ptr(), BPT,
                            out.data_ptr() + 4 * DIM * BPT * j, _lib.DTYPE_F32, found.data_ptr() + seg[j], 0, 0, None) for j in range(N_TABLES)]

                    def call():
                        for p in per:
                            L.mee_find_pooled_tiered(*p)
                for _ in range(10):
                    call()
                torch.cuda.synchronize(dev)
                ts = []
                for _ in range(args.chunks):
                    e0.record()
                    for _ in range(args.reps):
                        call()
                    e1.record()
                    torch.cuda.synchronize(dev)
                    ts.append(e0.elapsed_time(e1) * 1e3 / args.reps)
                results[f"{shape}, {dist}, {placement}"] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "keys": n,
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
    print(f"\n{N_TABLES} members, dim {DIM}, {BPT} bags per table, {args.hot} hot + {args.cold} cold keys per member; {args.passes} passes x {args.chunks} chunks x {args.reps} calls; "
          f"loop on {'the library at ' + args.loop_lib if args.loop_lib else 'this build'}")
    print("| bags, keys, placement | loop us (per pass) | group us (per pass) | flat us (per pass) | larger pass-to-pass spread | loop / group | faster by more than the spread |")
    print("|---|---|---|---|---|---|---|")
    for row, sides in table.items():
        assert len(sums[row]) == 1, f"{row}: the loop and the one launch disagree on the rows or the found mask: {sums[row]}"
        spread = {s: (max(v) - min(v)) / statistics.mean(v) for s, v in sides.items()}
        lo, gr = statistics.mean(sides["loop"]), statistics.mean(sides["group"])
        worst = max(spread["loop"], spread["group"])
        fmt = lambda v: " / ".join(f"{x:.1f}" for x in v)  # noqa: E731
        print(f"| {row} | {fmt(sides['loop'])} | {fmt(sides['group'])} | {fmt(sides['flat']) if 'flat' in sides else '—'} | {worst * 100:.1f} % | {lo / gr:.2f} | "
              f"{'yes' if (lo - gr) / lo > worst else 'NO'} |")


if __name__ == "__main__":
    child() if args.side else driver()
