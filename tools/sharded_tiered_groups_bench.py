"""The owner's side of a sharded collection of hot/cold pairs (mee_group_find_pooled_tiered_jagged, ShardedTieredTableGroup) on the collection of
tools/tiered_groups_bench.py: 26 pairs, dim 64, 2048 bags per table, hot tier in HBM, cold rows in pinned host memory, uniform keys.

launch rows (device time by events; ctypes calls with arguments prepared once), per bag shape (mean length 8: four bags per wave; mean 20: a wave per bag)
and placement (every lookup hot; a tenth cold):
  regular        ONE mee_group_find_pooled_tiered launch over the 26 x 2048 bags — also on another build of the library (--parent-lib: the parent commit's)
  jagged-regular ONE mee_group_find_pooled_tiered_jagged launch on the same bags with the map [0, B, 2B, …]: what the binary search over member_bags costs
  jagged-runs    ONE jagged launch on a run list such as the owner of a 2-rank world receives: per member the bags of two sources, each key kept with
                 probability 1/2 (as a hash owner keeps it), empty runs dropped — so the members' run counts differ
  loop-runs      26 mee_find_pooled_tiered launches on the same runs, member by member: what an owner would otherwise do
The rows of one process take turns inside ONE loop (a chunk of `reps` calls of each row per round).  Without a sub-command the tool is the driver: per pass
one fresh process on the parent's library and one on this build with the regular rows alone (like with like), and one on this build with all rows,
`--passes` passes; it prints per row the median of each pass and the pass-to-pass spread, and the ratios.

step: world 1 over the nccl backend (RCCL): find_pooled + Adagrad apply_pooled of ONE ShardedTieredTableGroup against the loop of 26
      ShardedLookupTable-over-pair find_pooled + apply_adagrad(grad_index=) calls on the same bags, the two alternating; host-clock times that end in a
      device synchronise, and the collectives each side issues per step.

usage: python tools/sharded_tiered_groups_bench.py [--parent-lib PATH] [--passes 2] [--chunks 7] [--reps 20] [--hot KEYS] [--cold KEYS]
       python tools/sharded_tiered_groups_bench.py step [--hot KEYS] [--cold KEYS]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("what", nargs="?", choices=["launch", "step"], default=None)
ap.add_argument("--rows", choices=["all", "regular"], default="all", help="launch: `regular` is what an older build of the library can run")
ap.add_argument("--parent-lib", default=None, help="driver: the parent commit's library for the regular rows")
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--chunks", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--hot", type=int, default=200_000, help="hot keys per member")
ap.add_argument("--cold", type=int, default=50_000, help="cold keys per member")
args = ap.parse_args()
N_TABLES, DIM, BPT = 26, 64, 2048
SHAPES = {"mean 8": (1, 15), "mean 20": (12, 28)}      # bag lengths drawn uniformly from [lo, hi]
PLACEMENTS = (("all hot", 1.0), ("a tenth cold", 0.9))


def make_pairs(dev, optimizer=0, max_batch=None):
    import torch

    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, _lib, synth
    kw = dict(optimizer=OPT_ADAGRAD, initial_accumulator=0.1) if optimizer else {}
    mb = max_batch or max(args.hot, args.cold)
    hots, colds, hot_keys, cold_keys = [], [], [], []
    for j in range(N_TABLES):
        hots.append(LookupTable(int(args.hot / 0.75), DIM, device=dev, max_batch=mb, **kw))
        colds.append(LookupTable(int(args.cold / 0.75), DIM, device=dev, max_batch=mb, value_memory=_lib.MEM_HOST_PINNED, **kw))
        for t, stream, count, keep in ((hots[-1], 100 + j, args.hot, hot_keys), (colds[-1], 200 + j, args.cold, cold_keys)):
            k = synth.keys_t(stream, 0, count, dev)
            for s in range(0, count, mb):
                t.insert(k[s:s + mb], synth.rows_t(k[s:s + mb], DIM, 2))
            keep.append(k)
    torch.cuda.synchronize(dev)
    return hots, colds, hot_keys, cold_keys


def draw_keys(g, dev, seg, hot_keys, cold_keys, hot_share):
    """keys for the member segments seg[j] .. seg[j + 1]: uniform over the member's hot keys, a share 1 - hot_share of the positions from its cold keys"""
    import torch
    keys = torch.empty(seg[-1], dtype=torch.int64, device=dev)
    for j in range(N_TABLES):
        m = seg[j + 1] - seg[j]
        k = hot_keys[j][(torch.rand(m, device=dev, generator=g) * args.hot).long().clamp(0, args.hot - 1)]
        if hot_share < 1.0:
            cold = torch.rand(m, device=dev, generator=g) >= hot_share
            k = torch.where(cold, cold_keys[j][(torch.rand(m, device=dev, generator=g) * args.cold).long().clamp(0, args.cold - 1)], k)
        keys[seg[j]:seg[j + 1]] = k
    return keys


def launch():
    import torch

    from meepoembedding_amd import TableGroup, _lib
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    g = torch.Generator(device=dev)
    hots, colds, hot_keys, cold_keys = make_pairs(dev)
    hot_group, cold_group = TableGroup(hots), TableGroup(colds)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    rows, keep = {}, []      # row name -> call; `keep` holds the tensors the prepared pointers name
    for shape, (lo, hi) in SHAPES.items():
        for placement, hot_share in PLACEMENTS:
            g.manual_seed(len(shape) + lo + int(hot_share * 10))      # every process draws the same bags and keys
            lens = torch.randint(lo, hi + 1, (N_TABLES * BPT,), device=dev, generator=g)
            off = torch.cat([zero, torch.cumsum(lens, 0)])
            n = int(off[-1])
            keys = draw_keys(g, dev, off[::BPT].tolist(), hot_keys, cold_keys, hot_share)
            out, found = torch.empty((N_TABLES * BPT, DIM), device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            keep += [off, keys, out, found]
            a = (hot_group._h, cold_group._h, keys.data_ptr(), n, off.data_ptr(), BPT, out.data_ptr(), _lib.DTYPE_F32, found.data_ptr(), 0, 0, None)
            rows[f"regular, {shape}, {placement}"] = lambda a=a: L.mee_group_find_pooled_tiered(*a)
            if args.rows == "regular":
                continue
            mb = torch.arange(N_TABLES + 1, dtype=torch.int64, device=dev) * BPT
            out2 = torch.empty_like(out)
            b = (hot_group._h, cold_group._h, keys.data_ptr(), n, off.data_ptr(), N_TABLES * BPT, mb.data_ptr(), out2.data_ptr(), found.data_ptr(), 0, 0, None)
            rows[f"jagged-regular, {shape}, {placement}"] = lambda b=b: L.mee_group_find_pooled_tiered_jagged(*b)
            _lib.check(L.mee_group_find_pooled_tiered(*a))
            _lib.check(L.mee_group_find_pooled_tiered_jagged(*b))
            assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), "the jagged launch at the regular map differs from the regular launch"
            # the run list of a 2-rank owner: two sources' bags per member, every key kept with probability 1/2, empty runs dropped
            full = torch.randint(lo, hi + 1, (N_TABLES, 2 * BPT), device=dev, generator=g)
            kept = torch.binomial(full.float(), torch.full_like(full, 0.5, dtype=torch.float32), generator=g).long()
            counts = (kept > 0).sum(dim=1)
            run_len = kept[kept > 0]      # (row-major: member by member, source 0's bags in front of source 1's)
            roff = torch.cat([zero, torch.cumsum(run_len, 0)])
            rmb = torch.cat([zero, torch.cumsum(counts, 0)])
            n_runs, rn = int(rmb[-1]), int(roff[-1])
            seg = roff[rmb].tolist()
            rkeys = draw_keys(g, dev, seg, hot_keys, cold_keys, hot_share)
            o1, o2 = torch.empty((n_runs, DIM), device=dev), torch.empty((n_runs, DIM), device=dev)
            f1 = torch.empty(rn, dtype=torch.uint8, device=dev)
            c = (hot_group._h, cold_group._h, rkeys.data_ptr(), rn, roff.data_ptr(), n_runs, rmb.data_ptr(), o1.data_ptr(), f1.data_ptr(), 0, 0, None)
            rows[f"jagged-runs, {shape}, {placement}"] = lambda c=c: L.mee_group_find_pooled_tiered_jagged(*c)
            rb = rmb.tolist()
            offs = [(roff[rb[j]:rb[j + 1] + 1] - seg[j]).contiguous() for j in range(N_TABLES)]
            per = [(hots[j]._h, colds[j]._h, rkeys.data_ptr() + 8 * seg[j], seg[j + 1] - seg[j], offs[j].data_ptr(), rb[j + 1] - rb[j],
                    o2.data_ptr() + 4 * DIM * rb[j], _lib.DTYPE_F32, f1.data_ptr() + seg[j], 0, 0, None) for j in range(N_TABLES)]

            def loop(per=per):
                for p in per:
                    L.mee_find_pooled_tiered(*p)
            rows[f"loop-runs, {shape}, {placement}"] = loop
            keep += [mb, out2, run_len, roff, rmb, rkeys, o1, o2, f1, offs]
            _lib.check(L.mee_group_find_pooled_tiered_jagged(*c))
            loop()
            assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), "the jagged launch on the runs differs from the loop over the pairs"
            print(f"{shape}, {placement}: {n} keys in {N_TABLES * BPT} bags; {rn} keys in {n_runs} runs, {int(counts.min())} .. {int(counts.max())} runs per member", flush=True)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {name: [] for name in rows}
    for r in range(2 + args.chunks):      # 2 warm-up rounds; the rows take turns inside the one loop
        for name, call in rows.items():
            e0.record()
            for _ in range(args.reps):
                call()
            e1.record()
            torch.cuda.synchronize(dev)
            if r >= 2:
                ts[name].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    print("RESULT " + json.dumps({name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in ts.items()}), flush=True)


def step():
    import numpy as np
    import torch
    import torch.distributed as dist

    from meepoembedding_amd import Router, TieredLookupTable, TieredTableGroup
    from meepoembedding_amd.sharded import ShardedLookupTable, ShardedTieredTableGroup
    dev = torch.device("cuda", 0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29536")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    n_max = 1 << 20
    hots, colds, hot_keys, cold_keys = make_pairs(dev, optimizer=1, max_batch=n_max)
    pairs = [TieredLookupTable(h, c) for h, c in zip(hots, colds)]
    router = Router(1, n_max, device=dev)
    singles = [ShardedLookupTable(p, router) for p in pairs]
    sg = ShardedTieredTableGroup(TieredTableGroup(pairs, max_apply_batch=n_max), router)
    g = torch.Generator(device=dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    for B in (256, BPT):
        for placement, hot_share in PLACEMENTS:
            g.manual_seed(B + int(hot_share * 10))
            lens = torch.randint(1, 16, (N_TABLES * B,), device=dev, generator=g)
            off = torch.cat([zero, torch.cumsum(lens, 0)])
            n = int(off[-1])
            o = off[::B].tolist()
            keys = draw_keys(g, dev, o, hot_keys, cold_keys, hot_share)
            grads = torch.randn(N_TABLES * B, DIM, device=dev, generator=g) * 0.01
            bag_of = torch.repeat_interleave(torch.arange(N_TABLES * B, device=dev), lens)
            segs = [(keys[o[j]:o[j + 1]].contiguous(), (off[j * B:(j + 1) * B + 1] - o[j]).contiguous(), grads[j * B:(j + 1) * B].contiguous(),
                     (bag_of[o[j]:o[j + 1]] - j * B).contiguous()) for j in range(N_TABLES)]

            def loop_step():
                for sh, (k, bo, gr, gi) in zip(singles, segs):
                    sh.find_pooled(k, bo, "sum")
                    sh.apply_adagrad(k, gr, 0.01, grad_index=gi)

            def group_step():
                sg.find_pooled(keys, off, "sum")
                sg.apply_pooled(keys, off, grads, bag_of, "adagrad", 0.01)

            times = {"loop": [], "group": []}
            for it in range(3 + 11):      # 3 warm-up rounds, then 11 timed ones, the two forms alternating
                for name, fn in (("loop", loop_step), ("group", group_step)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it >= 3:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            c0, l0 = sg.collectives, sum(s.collectives for s in singles)
            group_step()
            loop_step()
            torch.cuda.synchronize()
            for name, ts in times.items():
                ts = np.array(ts)
                print(f"{N_TABLES} x {B} bags x ~8 keys ({n} keys), {placement}, world 1, {name}: median {np.median(ts):.3f} ms, min {ts.min():.3f}, max {ts.max():.3f} "
                      f"over {ts.size} steps")
            print(f"B {B}, {placement}: collectives per step: group {sg.collectives - c0}, loop {sum(s.collectives for s in singles) - l0}; "
                  f"median loop / group = {np.median(times['loop']) / np.median(times['group']):.2f}", flush=True)
    dist.destroy_process_group()


def driver():
    table = {}      # row -> build -> [median per pass]
    for p in range(args.passes):
        # the builds take turns, a fresh process each; (a) compares like with like: the regular rows alone on either build
        for build in (["parent", "this-regular"] if args.parent_lib else []) + ["this"]:
            env = dict(os.environ)
            cmd = [sys.executable, os.path.abspath(__file__), "launch", "--chunks", str(args.chunks), "--reps", str(args.reps), "--hot", str(args.hot),
                   "--cold", str(args.cold)]
            if build == "parent":
                env.update(MEE_LIB_PATH=os.path.abspath(args.parent_lib), MEE_LIB_OLDER_BUILD="1")
            if build != "this":
                cmd += ["--rows", "regular"]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            line = [x for x in res.stdout.splitlines() if x.startswith("RESULT ")]
            if res.returncode != 0 or not line:
                print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"{build} build, pass {p + 1} failed with exit status {res.returncode}")
            if build == "this" and p == 0:
                print("\n".join(x for x in res.stdout.splitlines() if not x.startswith("RESULT ")))
            for row, r in json.loads(line[0][7:]).items():
                table.setdefault(row, {}).setdefault(build, []).append(r["median_us"])
                print(f"pass {p + 1} {build:6s} {row}: median {r['median_us']:.1f} us (chunks {r['min_us']:.1f} .. {r['max_us']:.1f})", flush=True)
    fmt = lambda v: " / ".join(f"{x:.1f}" for x in v)  # noqa: E731
    spread = lambda v: (max(v) - min(v)) / statistics.mean(v)  # noqa: E731
    print(f"\n{N_TABLES} pairs, dim {DIM}, {BPT} bags per table, {args.hot} hot + {args.cold} cold keys per member; {args.passes} passes x {args.chunks} chunks x {args.reps} calls")
    print("\n(a) the regular launch, parent build against this build (a process with the regular rows alone on either)\n"
          "| bags, placement | parent us (per pass) | this us (per pass) | this, beside the other rows | parent's pass-to-pass spread | this / parent |\n|---|---|---|---|---|---|")
    for row, b in table.items():
        if row.startswith("regular") and "parent" in b:
            print(f"| {row[9:]} | {fmt(b['parent'])} | {fmt(b['this-regular'])} | {fmt(b['this'])} | {spread(b['parent']) * 100:.1f} % | "
                  f"{statistics.mean(b['this-regular']) / statistics.mean(b['parent']):.3f} |")
    print("\n(b) the jagged launch at the regular map against the regular launch, this build, same bags\n| bags, placement | regular us | jagged us | larger spread | jagged / regular |\n|---|---|---|---|---|")
    for row, b in table.items():
        if row.startswith("jagged-regular"):
            reg = table["regular" + row[14:]]["this"]
            print(f"| {row[16:]} | {fmt(reg)} | {fmt(b['this'])} | {max(spread(reg), spread(b['this'])) * 100:.1f} % | {statistics.mean(b['this']) / statistics.mean(reg):.3f} |")
    print("\n(c) the jagged launch on a 2-rank owner's run list against the loop of 26 pair launches\n| source bags, placement | loop us | jagged us | larger spread | loop / jagged |\n|---|---|---|---|---|")
    for row, b in table.items():
        if row.startswith("jagged-runs"):
            lo = table["loop-runs" + row[11:]]["this"]
            print(f"| {row[13:]} | {fmt(lo)} | {fmt(b['this'])} | {max(spread(lo), spread(b['this'])) * 100:.1f} % | {statistics.mean(lo) / statistics.mean(b['this']):.2f} |")


if __name__ == "__main__":
    {"launch": launch, "step": step, None: driver}[args.what]()
