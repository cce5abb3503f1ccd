"""usage (GPU box):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 tools/sharded_groups_profile.py kernels
    python3 tools/sharded_groups_profile.py step
kernels: mee_segment_counts / mee_regroup next to the partition's three kernels at 1M keys, 26 tables, dim 64, 8 owners emulated in one process (the
         owner's inbox = segment 0 of the same source batch from all 8 sources, about 1M keys).
step:    world 1 over the nccl backend: find + Adagrad apply of ONE ShardedTableGroup call against a loop of 26 ShardedLookupTable calls on the same
         batch, alternating in one process; medians of host-clock times that end in a device synchronise."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from meepoembedding_amd import OPT_ADAGRAD, LookupTable, Router, TableGroup, synth

dev = torch.device("cuda", 0)
T, dim = 26, 64


def jagged(n, rng, stored):
    lens = rng.multinomial(n, np.ones(T) / T)
    keys = torch.from_numpy(stored[rng.integers(0, stored.size, n)]).to(dev)
    return keys, torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)


def kernels():
    G, n = 8, 1 << 20
    rng = np.random.default_rng(1)
    keys, off = jagged(n, rng, synth.keys_np(1, 0, 1 << 22))
    r = Router(G, n, device=dev)
    send, counts, perm = r.partition(keys)
    cells = r.segment_counts(perm, counts, off)
    c0 = int(counts[0])
    recv = send[:c0].repeat(G)
    recv_cells = cells[0:1].repeat(G, 1).contiguous()
    rows = torch.randn(recv.numel(), dim, device=dev)
    for it in range(20):
        send, counts, perm = r.partition(keys)
        cells = r.segment_counts(perm, counts, off)
        k_tm, order, off_tm = r.regroup(recv, recv_cells)
        g_tm = r.gather_rows(rows, order)
    torch.cuda.synchronize()
    assert int(cells.sum()) == n and int(off_tm[-1]) == recv.numel() and bool((k_tm == recv[order]).all())
    nr = recv.numel()
    print(f"n {n} T {T} G {G} dim {dim}: partition reads {8 * n} B twice and writes {16 * n} B; segment_counts makes {G * (T + 1)} searches in perm and writes "
          f"{8 * G * T} B; regroup over {nr} received keys reads {8 * nr + 8 * G * T} B and writes {16 * nr + 8 * (T + 1)} B = {24 * nr + 8 * G * T + 8 * (T + 1)} B; "
          f"gather_rows through order moves {nr * (8 + 2 * 4 * dim)} B")


def step():
    import torch.distributed as dist

    from meepoembedding_amd.sharded import ShardedLookupTable, ShardedTableGroup
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    rng = np.random.default_rng(2)
    stored = synth.keys_np(1, 0, 100_000)
    n_max = 1 << 20
    tables = []
    for j in range(T):
        t = LookupTable(1 << 18, dim, device=dev, optimizer=OPT_ADAGRAD, initial_accumulator=0.1, max_batch=n_max)
        t.insert(torch.from_numpy(stored).to(dev), torch.from_numpy(synth.rows_np(stored, dim, 2 + j)).to(dev))
        tables.append(t)
    router = Router(1, n_max, device=dev)
    singles = [ShardedLookupTable(t, router) for t in tables]
    sg = ShardedTableGroup(TableGroup(tables, max_apply_batch=n_max), router)
    for n in (1 << 16, 1 << 20):
        keys, off = jagged(n, rng, stored)
        grads = torch.randn(n, dim, device=dev) * 0.01
        o = off.tolist()
        segs = [(keys[o[j]:o[j + 1]].contiguous(), grads[o[j]:o[j + 1]].contiguous()) for j in range(T)]

        def loop_step():
            for sh, (k, g) in zip(singles, segs):
                sh.find(k)
                sh.apply_adagrad(k, g, 0.01)

        def group_step():
            sg.find(keys, off)
            sg.apply_adagrad(keys, off, grads, 0.01)

        times = {"loop": [], "group": []}
        for it in range(5 + 30):      # 5 warm-up rounds, then 30 timed ones, the two forms alternating
            for name, fn in (("loop", loop_step), ("group", group_step)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= 5:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        c0 = sg.collectives
        group_step()
        for name, ts in times.items():
            ts = np.array(ts)
            print(f"n {n} T {T} dim {dim} world 1 {name}: median {np.median(ts):.3f} ms, min {ts.min():.3f}, max {ts.max():.3f} over {ts.size} steps")
        print(f"n {n}: collectives per group step {sg.collectives - c0} (loop: {7 * T}); median loop / group = {np.median(times['loop']) / np.median(times['group']):.2f}")
    dist.destroy_process_group()


if __name__ == "__main__":
    {"kernels": kernels, "step": step}[sys.argv[1]]()
